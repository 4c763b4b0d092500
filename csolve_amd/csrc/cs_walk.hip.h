/* cs_walk.hip.h -- cs_walk_clauses: many instances of ONE clause model in one launch, a whole depth-first search per
 * wavefront (csgpu_solve_many_clauses; the walk is defined in csolve_gpu.h).
 *
 * For the models of kernel 6 (cs_propagate_clause_rounds, cs_kernels.hip.h: at most 512 clauses of any kind, resident in
 * registers).  What cs_dive_shave is to kernel 7, this is to kernel 6: the fixpoint is kernel 6's round loop -- the one
 * text of it, cs_rounds_body.hip.h -- and around it a wave draws an instance, runs its root node and walks its tree by
 * itself, with a private incumbent under MIN / MAX.
 *
 *   node      the current node lives in the wave's LDS slice (kernel 6's: n intervals and the round's flag word), where
 *             the fixpoint narrows it in place, and, as it was entered, in the wave's frame `depth` in device memory
 *   branch    the open variable with the smallest hi - lo, ties to the lowest index, "<obj>" included: every lane keeps
 *             the best of its own variables, then two wave minima (the width as a full 32-bit key, then the index among
 *             the lanes that hold that width); values in ascending order
 *   child     the node again (read back from its frame unless it was entered just now), x = value by lane 0 and, once
 *             the instance has a solution under MIN / MAX, dom[obj] = cs_objective_bound(sense, dom[obj], best): what
 *             kernel 6 does at node entry.  Then the rounds.  A bound that empties dom[obj] fails in the first round's
 *             check of the intervals: a node and a cut
 *   descend   a consistent child with open variables becomes the current node.  Unless the value was its parent's last,
 *             lane 0 writes {variable, next value} behind the parent's row and the child takes the next frame; else it
 *             takes the parent's frame
 *   solution  a consistent child without open variables.  ANY / ALL keep the first row and ANY leaves; MIN / MAX set
 *             best = dom[obj], overwrite the row and walk on
 *   pop       when the current node's values are used up; an empty stack ends the instance
 *
 * A frame is n + 1 entries of 8 bytes: the row in absolute bounds, each entry written and read back by the lane that owns
 * the variable (v mod 64), and {variable, next value}, lane 0's.  No fence, no atomic per node.  A pushed frame's level
 * values at least one variable, so at most n - 1 pushed frames and the current one are in use: n frames per wave; the
 * kernel compares the depth before it writes all the same (CSGPU_MANY_LIMIT rather than a write past the slice).
 *
 * Counters as cs_dive_shave's: nodes = children tried, cuts = inconsistent children, solutions, props = kernel 6's props
 * of the consistent children (per lane, reduced every 64 nodes and at the end), root_props = those of the root node.
 * max_nodes is compared before a child is tried.  Per-instance state beyond the node is scalars: best, have_best, the
 * counters, depth, variable, value.
 *
 * Work distribution: cs_dive_shave's tickets (cs_dive.hip.h), on the model's same counters; the wave barrier in front of
 * the draw is the one cs_dive_body.hip.h explains.  Device memory is written by plain vector stores and the one ticket
 * atomic.
 *
 * Checkpoints (cs_walk_resume, csgpu_solve_many_clauses_checkpointed / _resume): the same loop -- both kernels include
 * cs_walk_body.hip.h, with CS_WALK_CK 0 and 1 -- as cs_dive_resume is cs_dive_shave's.  An instance that stops at its
 * budget draws a slot of a pool (one relaxed atomic add by lane 0) and leaves there what the loop needs to go on at "try
 * value nv of variable bv on the node in frame depth":
 *
 *   slot = n + 1 frames of n + 1 entries (8 bytes each), bounds absolute as in the workspace
 *   frame 0           the header, lane 0's: entry 0 = {depth, CS_WALK_CK_MAGIC}, entry 1 = {best, have_best | objective << 1}
 *   frame 1 + d       pushed frame d (d < depth), exactly as in the workspace: the row, then {variable, next value}
 *   frame 1 + depth   the current node as it was entered, with {bv, nv} behind it
 *
 * The counters go to the instance's record as always and are read back from there; the incumbent travels in the header,
 * so a stopped MIN / MAX walk keeps the bound that makes the rest of its tree small.  A fresh instance walks in the wave's
 * workspace slice and copies its depth + 1 frames out when it stops (every lane the entries it wrote itself); a resumed
 * one uses the frames of its slot AS its stack, reads the current node back from frame depth (root = false, fresh =
 * false), and when it stops again writes only the header and {bv, nv}.  A resume launch needs no workspace.  The budget
 * of a resumed instance counts the nodes of this launch.  The header's objective must be the call's: a checkpoint made
 * under ALL has no incumbent to go on with under MIN, and one made under ANY would never have been written.
 *
 * Up to k solutions (cs_walk_upto, csgpu_solve_many_clauses_upto / _upto_checkpointed / _upto_resume): the same loop a
 * third time, with CS_WALK_CK 1 and CS_WALK_UPTO 1.  The instance walks the ALL walk (sense 0, "<obj>" an ordinary
 * variable, no incumbent) and leaves right after its k-th solution, DONE; solution j (0-based, walk order) goes to row
 * (inst * k + j) of io.solutions, an index of 64 bits, every lane the variables it owns.  A root row that is a solution is
 * row 0.  The header's code is CS_WALK_CK_UPTO, so a checkpoint of this kernel and one of cs_walk_resume refuse each
 * other (CSGPU_MANY_BAD_SLOT).  A resumed instance continues its rows at index `solutions` of its record, with the k of
 * the call; one that holds k already ends DONE before it tries a node, with only its status word and slot number
 * written.
 *
 * Restarts (cs_walk_restart, csgpu_solve_many_clauses_restarts): the same loop a fourth time, CS_WALK_RESTART 1, ANY only
 * and without checkpoints; what cs_dive_restart is to cs_dive_shave.  A node tries its values in the rotation of
 * cs_many_start / cs_many_rotated (cs_arith.h) that depends on (seed of the instance, run, variable), and after more than
 * threshold x restart_base failed children the walk starts again from the root node's fixpoint with run + 1 and the next
 * Luby threshold.  Counters and the budget run over all runs; a restart costs no node and no rounds.  Frame 0 cannot keep
 * the root: a node's last-value child takes its parent's frame.  So the call has n + 1 frames per wave, the walk stays
 * below frame n, and frame n holds the root fixpoint, every lane the entries it owns.  Everything new is a scalar.
 *
 * Every solution (cs_walk_stream, csgpu_solve_many_clauses_stream): the same loop a fifth time, CS_WALK_CK 1 and
 * CS_WALK_STREAM 1, the ALL walk of cs_walk_upto.  A solution is appended to one output stream shared by all waves
 * (cs_dive_out, as cs_dive_stream): lane 0 adds 1 to one 64-bit word (relaxed, agent scope), the old value is the row --
 * every lane stores the variables it owns there, lane 0 the owner -- unless it is past the capacity: then the child is NOT
 * counted (the draw stands before nodes and props move) and the instance stops with CSGPU_MANY_FULL through the budget's
 * checkpoint code, {bv, nv} with nv that very value, so the next call tries it again; the node is intact in its frame.
 * Fresh or resumed is a fact per instance (slots[i] == -2 or >= 0).  The header's code is CS_WALK_CK_STREAM.  A wave that
 * finds the stream full when it has drawn a ticket does not walk.  Three atomics: ticket, pool, stream.
 *
 * Start incumbents (cs_walk_from, csgpu_solve_many_clauses_from / _from_resume): the same loop a sixth time, CS_WALK_CK 1
 * and CS_WALK_FROM 1, the MIN / MAX walk of cs_walk_resume.  A fresh instance with start[inst].have != 0 begins with
 * have_best, best = start[inst].best -- dom[obj] of its root row takes the objective bound before the root node's rounds
 * -- and only a solution of the instance's own is reported (io.best iff solutions > 0; the row is written at solutions
 * only anyway).  The header's code is the objective's, so a checkpoint of this kernel and one of cs_walk_resume continue
 * under either.  ck.capacity == 0: no pool, as cs_walk_upto.  It is what lets a stopped MIN / MAX walk be spread: see the
 * fan-out below.
 *
 * Variable orders and halving (cs_walk_order, csgpu_solve_many_clauses_ordered): the same loop a seventh time,
 * CS_WALK_ORDER 1, without checkpoints, pools, the stream or restarts.  The two wave minima run over cs_order_key(order, d)
 * (cs_arith.h, the engine's key) in place of the width, and a node whose branching variable has more than split_width
 * values makes two children, [lo, mid] and [mid + 1, hi], in place of one per value.  Kind and mid are scalars read from
 * the node as it was entered; a frame's {variable, next} keeps its 8 bytes, next = mid + 1 for a halving node, whose kind
 * is read back from the frame's row.  A pushed halving parent values no variable, so the frames per wave are the host's
 * bound n + sum of h(v), not n.
 *
 * The ordered walk with checkpoints (cs_walk_order_resume, csgpu_solve_many_clauses_ordered_checkpointed / _resume): the
 * same loop an eighth time, CS_WALK_CK 1 and CS_WALK_ORDER 1.  With F = io.frames, the host's bound above:
 *
 *   slot = F + 1 frames of n + 1 entries (8 bytes each), bounds absolute
 *   frame 0           the header: entry 0 = {depth, CS_WALK_CK_MAGIC_ORDER}, entry 1 = {best, have_best | code << 1},
 *                     code = objective | order << 3
 *   frame 1 + d       pushed frame d (d < depth <= F - 1): the row, then {variable, next value or mid + 1}
 *   frame 1 + depth   the current node as it was entered, with {bv, nv} behind it
 *
 * F + 1 and not n + 1 frames, because up to F - 1 parents are pushed under the current node.  A resume under another
 * objective or another order would walk another tree: its code differs, CSGPU_MANY_BAD_SLOT.  A pool is made for one
 * split_width (the host compares it), which fixes F for the fresh and the resume launch.  The halving count goes on from
 * ord.halvings[inst] as the other counters go on from the record; a walk stopped between the two halves of a node finds
 * nv == mid + 1 in its frame and counts the parent once.  cs_walk_children / cs_walk_fanout do not read these slots (the
 * host refuses the pool): a fan-out of halves has to account for `halvings`, which cs_walk_order_children /
 * cs_walk_order_fanout below do.
 *
 * The ordered walk from a start incumbent (cs_walk_order_from, csgpu_solve_many_clauses_ordered_from / _from_resume): the
 * same loop a ninth time, CS_WALK_CK 1, CS_WALK_ORDER 1 and CS_WALK_FROM 1 -- cs_walk_order_resume's slots and code,
 * cs_walk_from's `start`, own-solutions report and "ck.capacity == 0: no pool".  It walks the children that
 * cs_walk_order_fanout makes of a stopped MIN / MAX walk.
 *
 * Past 512 clauses (cs_walk_wide, cs_walk_wide_resume; csgpu_solve_many_clauses_wide / _wide_checkpointed / _wide_resume):
 * the same loop a tenth and an eleventh time, CS_WALK_WIDE 1 with CS_WALK_CK 0 and 1.  The 512 are the register file's,
 * not the walk's: the rounds read rec[q], lit0[q], lit1[q], and here those are LDS reads of one block per workgroup --
 * T.clause_by_kind, then T.lit -- staged before the ticket loop behind one __syncthreads() (cs_walk_body.hip.h), with the
 * round loop of cs_rounds_wide_body.hip.h: a run-time slot loop over ceil(n_clauses / 64) slots, clause lane + 64 q in
 * slot q.  That is kernel 6's lane-to-clause assignment and slot order, so on a model of at most 512 clauses every field
 * of the answer, props included, is cs_walk_clauses's.  Dynamic LDS per workgroup: 16 (n_clauses + n_lits) bytes and the
 * four slices.  The switch table, with the two new rows:
 *                        CS_WALK_CK  UPTO  RESTART  STREAM  FROM  ORDER  WIDE
 *   cs_walk_clauses          0        0      0        0      0     0      0
 *   cs_walk_resume           1        0      0        0      0     0      0
 *   cs_walk_upto             1        1      0        0      0     0      0
 *   cs_walk_restart          0        0      1        0      0     0      0
 *   cs_walk_stream           1        0      0        1      0     0      0
 *   cs_walk_from             1        0      0        0      1     0      0
 *   cs_walk_order            0        0      0        0      0     1      0
 *   cs_walk_order_resume     1        0      0        0      0     1      0
 *   cs_walk_order_from       1        0      0        0      1     1      0
 *   cs_walk_wide             0        0      0        0      0     0      1
 *   cs_walk_wide_resume      1        0      0        0      0     0      1
 * A slot of cs_walk_wide_resume is cs_walk_resume's (n + 1 frames, CS_WALK_CK_MAGIC, the objective as its code); the host
 * keeps the pools apart by a kind of their own, so that no entry of the older families is handed a model it refuses.
 * Resources (-Rpass-analysis=kernel-resource-usage, gfx950) are in DESIGN.md 3.10. */
#ifndef CS_WALK_HIP_H
#define CS_WALK_HIP_H

#include "cs_kernels.hip.h"
#include "cs_step.hip.h"
#include "cs_dive.hip.h"

struct cs_walk_io {
  const cs_val *roots;     /* [count][n] */
  const cs_val *root_dom;  /* [n]: the model's root domains, which a root row must lie inside */
  int count;
  int all;                 /* 0: leave at the first solution (ANY), 1: walk the whole tree (ALL, MIN, MAX); cs_walk_upto does
                              not read it */
  int sense;               /* cs_objective_bound's: 0 none (ANY / ALL), 1 minimise, 2 maximise */
  int obj_var;             /* "<obj>" under MIN / MAX, else -1 */
  long long max_nodes;
  cs_dive_result *results; /* [count] */
  int *solutions;          /* [count][n] or NULL: the first solution (ANY / ALL), the best one so far (MIN / MAX);
                              cs_walk_upto: [count][k][n] or NULL, the first k in walk order */
  int *best;               /* [count] or NULL: MIN / MAX, instances with a solution */
  cs_val *stack;           /* [waves][frames][n + 1] */
  int frames;
  unsigned *tickets;       /* CS_DIVE_SHARDS counters, zero between launches */
};

template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_clauses(cs_tables T, cs_walk_io io) {
#define CS_WALK_CK 0
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 0
#define CS_WALK_ORDER 0
#define CS_WALK_WIDE 0
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

#define CS_WALK_CK_MAGIC 0x77636b70 /* header entry 0 .hi of a slot that holds a clause checkpoint (not CS_DIVE_CK_MAGIC) */
#define CS_WALK_CK_UPTO 4           /* the header's code of an up-to-k checkpoint (cs_walk_upto): beside the objectives 0 .. 3 */
#define CS_WALK_CK_STREAM 5         /* that of a stream checkpoint (cs_walk_stream) */

/* the checkpoint pool and the slot numbers of a call (cs_walk_resume) */
struct cs_walk_ck {
  cs_val *pool;             /* [capacity][n + 1][n + 1]; cs_walk_order_resume: [capacity][io.frames + 1][n + 1] */
  unsigned long long *next; /* slots handed out since the last reset (it counts on past capacity) */
  int capacity;             /* cs_walk_upto: 0 = no pool (pool, next and slots are not touched) */
  int resume;               /* 0: fresh instances from io.roots; 1: instance i goes on from slot slots[i] */
  int code;                 /* the call's objective, 0 ANY .. 3 MAX, CS_WALK_CK_UPTO or CS_WALK_CK_STREAM: a checkpoint goes on
                               under the one it was made under; cs_walk_order_resume: objective | order << 3 */
  int *slots;               /* [count]: the slot of an instance stopped with a checkpoint, else -1 */
};

/* the same with checkpoints: fresh instances (ck.resume == 0) or the instances of ck.slots going on */
template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_resume(cs_tables T, cs_walk_io io, cs_walk_ck ck) {
#define CS_WALK_CK 1
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 0
#define CS_WALK_ORDER 0
#define CS_WALK_WIDE 0
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

/* the same again, leaving an instance right after its `upto`-th solution and keeping all of them (upto >= 1) */
template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_upto(cs_tables T, cs_walk_io io, cs_walk_ck ck, int upto) {
#define CS_WALK_CK 1
#define CS_WALK_UPTO 1
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 0
#define CS_WALK_ORDER 0
#define CS_WALK_WIDE 0
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

/* the ANY walk with a seeded value order and Luby restarts (csgpu_solve_many_clauses_restarts): `rs` is cs_dive_restart's;
 * io.frames is n + 1, the last frame the root node's fixpoint */
template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_restart(cs_tables T, cs_walk_io io, cs_dive_rs rs) {
#define CS_WALK_CK 0
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 1
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 0
#define CS_WALK_ORDER 0
#define CS_WALK_WIDE 0
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

/* the ALL walk that appends every solution to `out` (cs_dive_stream's descriptor) and steps back when there is no room;
 * ck.resume and io.all are not read: ck.slots[i] says per instance whether it starts (-2), goes on (>= 0) or is finished
 * (anything else) */
template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_stream(cs_tables T, cs_walk_io io, cs_walk_ck ck, cs_dive_out out) {
#define CS_WALK_CK 1
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 1
#define CS_WALK_FROM 0
#define CS_WALK_ORDER 0
#define CS_WALK_WIDE 0
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

/* the incumbent an instance of cs_walk_from starts with (csgpu_many_start): `best` counts only where `have` is not 0 */
struct cs_walk_start {
  int best;
  int have;
};

/* the MIN / MAX walk of cs_walk_resume whose fresh instances may start with an incumbent they did not find themselves, and
 * which reports only solutions of their own (csgpu_solve_many_clauses_from / _from_resume); ck.capacity == 0: no pool */
template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_from(cs_tables T, cs_walk_io io, cs_walk_ck ck, const cs_walk_start *start) {
#define CS_WALK_CK 1
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 1
#define CS_WALK_ORDER 0
#define CS_WALK_WIDE 0
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

/* what cs_walk_order takes beside cs_walk_clauses's arguments (csgpu_many_order_options) */
struct cs_walk_ord {
  int order;           /* cs_order_key's: 0 none, 1 smallest domain, 2 largest domain, 3 smallest value, 4 largest value */
  int split_width;     /* >= 1: a branching variable of more values is halved, not enumerated */
  long long *halvings; /* [count] or NULL: parents split in two; cs_walk_order_resume: [count], read back by a resumed instance */
};

/* cs_walk_clauses's walk under one of the engine's five variable orders, with intervals of more than split_width values
 * halved (csgpu_solve_many_clauses_ordered; the walk is defined in csolve_gpu.h): the same loop a seventh time,
 * CS_WALK_ORDER 1 and every other switch 0.  A halving parent that is pushed values no variable, so io.frames is
 * n + sum of h(v) (csgpu_many_clauses_ordered_frames), computed on the host from the root domains */
template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_order(cs_tables T, cs_walk_io io, cs_walk_ord ord) {
#define CS_WALK_CK 0
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 0
#define CS_WALK_ORDER 1
#define CS_WALK_WIDE 0
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

#define CS_WALK_CK_MAGIC_ORDER 0x776f6b70 /* header entry 0 .hi of a slot of cs_walk_order_resume: F + 1 frames, not n + 1 */

/* cs_walk_order's walk with cs_walk_resume's checkpoints (csgpu_solve_many_clauses_ordered_checkpointed / _resume): the same
 * loop an eighth time, CS_WALK_CK 1 and CS_WALK_ORDER 1.  A slot is io.frames + 1 frames, ck.code objective | order << 3,
 * ord.halvings is required and read back by a resumed instance */
template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_order_resume(cs_tables T, cs_walk_io io, cs_walk_ck ck, cs_walk_ord ord) {
#define CS_WALK_CK 1
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 0
#define CS_WALK_ORDER 1
#define CS_WALK_WIDE 0
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

/* ---- a stopped ALL walk spread over the waves of the next launch (csgpu_many_clause_checkpoint_children / _fanout; the
 * fold is cs_dive_fold, which knows records only)
 *
 * What cs_dive_children / cs_dive_fanout (cs_dive.hip.h) are to a kernel-7 pool, for a clause pool: the same frames "node,
 * branching variable bv, next value" and the same walk order -- the values next .. node[bv].hi of the current node (frame
 * 1 + depth of the slot), then those of the frame below it, down to frame 1 -- but the bounds are absolute, the header is
 * a frame of its own (frame 0) and a domain may be 2^32 values wide, so a frame's count is taken in 64 bits.  A parent is
 * pushed only while it has values left, so every frame has a child.  Child (d, v) as a root row of its own is what the walk
 * makes of it: cs_walk_body.hip.h runs the root row and every child through the same text -- the node in the LDS slice,
 * then cs_rounds_body.hip.h -- and under ALL no incumbent touches the slice.  So the contribution of cs_dive_fold holds
 * here as well, props included.
 *
 * The ALL entries are ALL only: under MIN / MAX the private incumbent is sequential, a split would change the tree.  A
 * header whose code is not the one asked for (ALL's: ANY 0, MIN 2, MAX 3, CS_WALK_CK_UPTO, CS_WALK_CK_STREAM) is refused
 * like a slot without a checkpoint.
 * Not templated, one wave per instance, CS_DIVE_FAN_WAVES instances per workgroup, 64-bit row indices, no atomics.  A
 * slot is checked before anything that depends on it is read: a slot number outside the pool, a header without the magic,
 * a depth outside [0, n), another code, a frame whose bv is outside [0, n), whose node's bounds of bv lie outside the root
 * domain or whose next value is outside those bounds give -1, never a count.
 *
 * The same two kernels serve csgpu_many_clause_checkpoint_children_obj / _fanout_obj with `code` MIN's 2 or MAX's 3 in
 * place of ALL's 1 (a scalar; the ALL entries pass CS_WALK_CK_ALL and NULL for the starts): a stopped MIN / MAX walk's
 * untried children are independent sub-problems, and any known solution value is a valid bound for all of them.  The
 * fan-out then writes, beside each row, the incumbent it starts with: the strictly better of the header's and the
 * owner's (owner_start, NULL or [count]), lane 0's 8-byte store; the children are walked by cs_walk_from. */
#define CS_WALK_CK_ALL 1 /* the header's code of a checkpoint written under ALL (CS_OBJ_ALL) */

static __device__ __forceinline__ long long cs_walk_slot_children(int n, const cs_val *__restrict__ root_dom,
                                                                  const cs_val *__restrict__ pool, int capacity, int slot,
                                                                  int lane, int code) {
  if (slot < 0) return 0;
  if (slot >= capacity) return -1;
  const size_t fstride = (size_t)n + 1;
  const cs_val *base = pool + (size_t)slot * (fstride * fstride);
  const cs_val head = base[0];
  const int depth = __builtin_amdgcn_readfirstlane(head.lo);
  if (__builtin_amdgcn_readfirstlane(head.hi) != CS_WALK_CK_MAGIC || depth < 0 || depth >= n) return -1;
  if ((__builtin_amdgcn_readfirstlane(base[1].hi) >> 1) != code) return -1; /* have_best | code << 1 */
  long long mine = 0;
  bool bad = false;
  for (int d = lane; d <= depth && !bad; d += CS_WAVE) {
    const cs_val *f = base + fstride * (1 + (size_t)d);
    const cs_val meta = f[n];
    if (meta.lo < 0 || meta.lo >= n) {
      bad = true;
    } else {
      const cs_val node = f[meta.lo], r = root_dom[meta.lo];
      if (node.lo < r.lo || node.hi > r.hi || node.lo > node.hi || meta.hi < node.lo || meta.hi > node.hi)
        bad = true;
      else
        mine += (long long)node.hi - (long long)meta.hi + 1;
    }
  }
  if (__ballot(bad) != 0ull) return -1;
  for (int o = CS_WAVE / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o, CS_WAVE);
  return cs_dive_uniform(mine);
}

/* children[i] = the untried children of the clause checkpoint in slot slots[i]: 0 for slots[i] < 0, -1 for a refused slot */
__global__ __launch_bounds__(CS_DIVE_FAN_WAVES * CS_WAVE) void cs_walk_children(int n, const cs_val *__restrict__ root_dom,
                                                                                const cs_val *__restrict__ pool, int capacity,
                                                                                const int *__restrict__ slots, long long count,
                                                                                long long *__restrict__ children, int code) {
  const int lane = (int)(threadIdx.x % CS_WAVE);
  const long long i = (long long)blockIdx.x * CS_DIVE_FAN_WAVES + (long long)(threadIdx.x / CS_WAVE);
  if (i >= count) return;
  const int slot = __builtin_amdgcn_readfirstlane(slots[i]);
  const long long c = cs_walk_slot_children(n, root_dom, pool, capacity, slot, lane, code);
  if (lane == 0) children[i] = c;
}

/* rows[offsets[i] ..] = the children of instance i in walk order, in absolute bounds as the frames hold them, owner[row] =
 * i.  The instance is counted again first: it writes nothing unless offsets[i + 1] - offsets[i] is its count and its rows
 * lie inside [0, total) */
__global__ __launch_bounds__(CS_DIVE_FAN_WAVES * CS_WAVE) void cs_walk_fanout(int n, const cs_val *__restrict__ root_dom,
                                                                              const cs_val *__restrict__ pool, int capacity,
                                                                              const int *__restrict__ slots, long long count,
                                                                              const long long *__restrict__ offsets,
                                                                              long long total, cs_val *__restrict__ rows,
                                                                              int *__restrict__ owner, int code,
                                                                              const cs_walk_start *__restrict__ owner_start,
                                                                              cs_walk_start *__restrict__ start_out) {
  const int lane = (int)(threadIdx.x % CS_WAVE);
  const long long i = (long long)blockIdx.x * CS_DIVE_FAN_WAVES + (long long)(threadIdx.x / CS_WAVE);
  if (i >= count) return;
  const int slot = __builtin_amdgcn_readfirstlane(slots[i]);
  if (slot < 0) return;
  const long long mine = cs_walk_slot_children(n, root_dom, pool, capacity, slot, lane, code);
  const long long off = cs_dive_uniform(offsets[i]), end = cs_dive_uniform(offsets[i + 1]);
  if (mine <= 0 || off < 0 || end > total || end - off != mine) return;
  const size_t fstride = (size_t)n + 1;
  const cs_val *base = pool + (size_t)slot * (fstride * fstride);
  const int depth = __builtin_amdgcn_readfirstlane(base[0].lo);
  cs_walk_start st; /* what every child of this slot starts with: the header's incumbent, or the owner's better one */
  st.best = 0;
  st.have = 0;
  if (start_out != nullptr) {
    const int sense = code == 2 ? 1 : 2;
    st.have = __builtin_amdgcn_readfirstlane(base[1].hi) & 1;
    if (st.have != 0) st.best = __builtin_amdgcn_readfirstlane(base[1].lo);
    if (owner_start != nullptr) {
      const int ohave = __builtin_amdgcn_readfirstlane(owner_start[i].have);
      if (ohave != 0) {
        const int obest = __builtin_amdgcn_readfirstlane(owner_start[i].best);
        if (st.have == 0 || cs_objective_better(sense, cs_interval(obest, obest), st.best)) st.best = obest;
        st.have = 1;
      }
    }
  }
  long long row = off;
  for (int d = depth; d >= 0; d--) {
    const cs_val *f = base + fstride * (1 + (size_t)d);
    const cs_val meta = f[n];
    const int bv = __builtin_amdgcn_readfirstlane(meta.lo);
    const int next = __builtin_amdgcn_readfirstlane(meta.hi);
    const int hi = __builtin_amdgcn_readfirstlane(f[bv].hi);
    for (long long v = next; v <= (long long)hi && row < end; v++, row++) {
      cs_val *dst = rows + (size_t)row * (size_t)n;
      for (int x = lane; x < n; x += CS_WAVE) dst[x] = x == bv ? cs_interval((int)v, (int)v) : f[x];
      if (owner != nullptr && lane == 0) owner[row] = (int)i;
      if (start_out != nullptr && lane == 0) start_out[row] = st;
    }
  }
}

/* cs_walk_order's walk with checkpoints AND cs_walk_from's start incumbents (csgpu_solve_many_clauses_ordered_from /
 * _from_resume): the same loop a ninth time, CS_WALK_CK 1, CS_WALK_ORDER 1 and CS_WALK_FROM 1.  Fresh instances are
 * cs_walk_order_resume's MIN / MAX walk and may begin with start[inst] under cs_walk_from's own-solutions rule; the slots
 * are cs_walk_order_resume's (same magic, same code), so a checkpoint of either kernel goes on under the other.
 * ck.capacity == 0: no pool, and then ord.halvings may be NULL (nothing is resumed) */
template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_order_from(cs_tables T, cs_walk_io io, cs_walk_ck ck, cs_walk_ord ord,
                                                               const cs_walk_start *start) {
#define CS_WALK_CK 1
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 1
#define CS_WALK_ORDER 1
#define CS_WALK_WIDE 0
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

/* ---- a stopped ORDERED walk spread over the waves of the next launch (csgpu_many_clause_ordered_checkpoint_children /
 * _fanout; the records fold with cs_dive_fold, the best values with cs_walk_fold_best, the halving counts with
 * cs_walk_fold_halvings)
 *
 * What cs_walk_children / cs_walk_fanout are to a plain clause pool, for a pool of cs_walk_order_resume: a slot is
 * `frames` + 1 frames under CS_WALK_CK_MAGIC_ORDER, its code objective | order << 3.  The children of a frame {row f, bv,
 * next}, lo, hi = f[bv], are the walk's own (cs_walk_body.hip.h reads kind and mid back from the frame's row in the same
 * way), mid = (lo + hi) >> 1 in 64 bits:
 *   enumerating (hi - lo + 1 <= split_width), next in [lo, hi]   the rows bv = [v, v], v = next .. hi
 *   halving, next == mid + 1                                    one child, bv = [mid + 1, hi]
 *   halving, next == lo (the current node only)                 two children, [lo, mid] then [mid + 1, hi]
 * In the third case the walk had not yet counted the parent in `halvings` (it does when the first half is tried), so the
 * instance owes one halving that no record holds: unsplit = 1.  Walk order: the current node's children, then those of
 * the frame below it, down to frame 1.  A child as a root row of its own is what the walk makes of it -- the row narrowed,
 * then cs_rounds_body.hip.h, then the branching variable chosen anew -- so under ALL the fold is exact, `halvings`
 * included: owner + unsplit + the sum of the sub-instances'.  Under MIN / MAX (code's objective 2 or 3) the fan-out
 * writes the start incumbent of every row as cs_walk_fanout does, and the rows are walked by cs_walk_order_from.
 * One wave per instance, CS_DIVE_FAN_WAVES instances per workgroup, 64-bit counts and row indices, no atomics.  Everything
 * is compared before what depends on it is read; -1 (never a partial count) for a slot number outside the pool, another
 * magic, a depth outside [0, frames), another code, a frame whose bv is outside [0, n), whose bounds of bv are empty or
 * outside the root domain, an enumerating frame whose next is outside [lo, hi], a halving frame whose next is neither
 * mid + 1 nor (current node only) lo. */
static __device__ __forceinline__ long long cs_walk_order_slot_children(int n, int frames, int split_width,
                                                                        const cs_val *__restrict__ root_dom,
                                                                        const cs_val *__restrict__ pool, int capacity,
                                                                        int slot, int lane, int code, int *unsplit) {
  *unsplit = 0;
  if (slot < 0) return 0;
  if (slot >= capacity) return -1;
  const size_t fstride = (size_t)n + 1;
  const cs_val *base = pool + (size_t)slot * (((size_t)frames + 1) * fstride);
  const cs_val head = base[0];
  const int depth = __builtin_amdgcn_readfirstlane(head.lo);
  if (__builtin_amdgcn_readfirstlane(head.hi) != CS_WALK_CK_MAGIC_ORDER || depth < 0 || depth >= frames) return -1;
  if ((__builtin_amdgcn_readfirstlane(base[1].hi) >> 1) != code) return -1; /* have_best | code << 1 */
  long long mine = 0;
  bool bad = false, owes = false;
  for (int d = lane; d <= depth && !bad; d += CS_WAVE) {
    const cs_val *f = base + fstride * (1 + (size_t)d);
    const cs_val meta = f[n];
    if (meta.lo < 0 || meta.lo >= n) {
      bad = true;
    } else {
      const cs_val node = f[meta.lo], r = root_dom[meta.lo];
      if (node.lo < r.lo || node.hi > r.hi || node.lo > node.hi) {
        bad = true;
      } else if ((long long)node.hi - (long long)node.lo + 1 > (long long)split_width) { /* halves: lo < mid + 1 <= hi */
        const int mid = (int)(((long long)node.lo + (long long)node.hi) >> 1);
        if (meta.hi == mid + 1) {
          mine += 1;
        } else if (d == depth && meta.hi == node.lo) {
          mine += 2;
          owes = true;
        } else {
          bad = true;
        }
      } else if (meta.hi < node.lo || meta.hi > node.hi) {
        bad = true;
      } else {
        mine += (long long)node.hi - (long long)meta.hi + 1;
      }
    }
  }
  if (__ballot(bad) != 0ull) return -1;
  if (__ballot(owes) != 0ull) *unsplit = 1;
  for (int o = CS_WAVE / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o, CS_WAVE);
  return cs_dive_uniform(mine);
}

/* children[i] = the untried children of the ordered checkpoint in slot slots[i]: 0 for slots[i] < 0, -1 for a refused slot;
 * unsplit[i] = 1 where the current node is a halving one with neither half tried, else 0 (a refused slot: 0) */
__global__ __launch_bounds__(CS_DIVE_FAN_WAVES * CS_WAVE) void cs_walk_order_children(
    int n, int frames, int split_width, const cs_val *__restrict__ root_dom, const cs_val *__restrict__ pool, int capacity,
    const int *__restrict__ slots, long long count, long long *__restrict__ children, int *__restrict__ unsplit, int code) {
  const int lane = (int)(threadIdx.x % CS_WAVE);
  const long long i = (long long)blockIdx.x * CS_DIVE_FAN_WAVES + (long long)(threadIdx.x / CS_WAVE);
  if (i >= count) return;
  const int slot = __builtin_amdgcn_readfirstlane(slots[i]);
  int owes = 0;
  const long long c = cs_walk_order_slot_children(n, frames, split_width, root_dom, pool, capacity, slot, lane, code, &owes);
  if (lane == 0) {
    children[i] = c;
    unsplit[i] = c > 0 ? owes : 0;
  }
}

/* rows[offsets[i] ..] = the children of instance i in walk order, owner[row] = i and, under MIN / MAX, start_out[row] as
 * cs_walk_fanout writes it.  The instance is counted again first: it writes nothing unless offsets[i + 1] - offsets[i] is
 * its count and its rows lie inside [0, total) */
__global__ __launch_bounds__(CS_DIVE_FAN_WAVES * CS_WAVE) void cs_walk_order_fanout(
    int n, int frames, int split_width, const cs_val *__restrict__ root_dom, const cs_val *__restrict__ pool, int capacity,
    const int *__restrict__ slots, long long count, const long long *__restrict__ offsets, long long total,
    cs_val *__restrict__ rows, int *__restrict__ owner, int code, const cs_walk_start *__restrict__ owner_start,
    cs_walk_start *__restrict__ start_out) {
  const int lane = (int)(threadIdx.x % CS_WAVE);
  const long long i = (long long)blockIdx.x * CS_DIVE_FAN_WAVES + (long long)(threadIdx.x / CS_WAVE);
  if (i >= count) return;
  const int slot = __builtin_amdgcn_readfirstlane(slots[i]);
  if (slot < 0) return;
  int owes = 0;
  const long long mine = cs_walk_order_slot_children(n, frames, split_width, root_dom, pool, capacity, slot, lane, code, &owes);
  const long long off = cs_dive_uniform(offsets[i]), end = cs_dive_uniform(offsets[i + 1]);
  if (mine <= 0 || off < 0 || end > total || end - off != mine) return;
  const size_t fstride = (size_t)n + 1;
  const cs_val *base = pool + (size_t)slot * (((size_t)frames + 1) * fstride);
  const int depth = __builtin_amdgcn_readfirstlane(base[0].lo);
  cs_walk_start st; /* what every child of this slot starts with: the header's incumbent, or the owner's better one */
  st.best = 0;
  st.have = 0;
  if (start_out != nullptr) {
    const int sense = (code & 7) == 2 ? 1 : 2;
    st.have = __builtin_amdgcn_readfirstlane(base[1].hi) & 1;
    if (st.have != 0) st.best = __builtin_amdgcn_readfirstlane(base[1].lo);
    if (owner_start != nullptr) {
      const int ohave = __builtin_amdgcn_readfirstlane(owner_start[i].have);
      if (ohave != 0) {
        const int obest = __builtin_amdgcn_readfirstlane(owner_start[i].best);
        if (st.have == 0 || cs_objective_better(sense, cs_interval(obest, obest), st.best)) st.best = obest;
        st.have = 1;
      }
    }
  }
  long long row = off;
  for (int d = depth; d >= 0; d--) {
    const cs_val *f = base + fstride * (1 + (size_t)d);
    const cs_val meta = f[n];
    const int bv = __builtin_amdgcn_readfirstlane(meta.lo);
    const int next = __builtin_amdgcn_readfirstlane(meta.hi);
    const int lo = __builtin_amdgcn_readfirstlane(f[bv].lo), hi = __builtin_amdgcn_readfirstlane(f[bv].hi);
    const bool halves = (long long)hi - (long long)lo + 1 > (long long)split_width;
    const int mid = (int)(((long long)lo + (long long)hi) >> 1);
    /* child c of the frame is bv = [a, b]: a value each, or the halves that are left (next == lo: both) */
    const long long kids = halves ? (next == lo ? 2 : 1) : (long long)hi - (long long)next + 1;
    for (long long c = 0; c < kids && row < end; c++, row++) {
      int a, b;
      if (!halves) {
        a = b = (int)((long long)next + c);
      } else if (next == lo && c == 0) {
        a = lo;
        b = mid;
      } else {
        a = mid + 1;
        b = hi;
      }
      cs_val *dst = rows + (size_t)row * (size_t)n;
      for (int x = lane; x < n; x += CS_WAVE) dst[x] = x == bv ? cs_interval(a, b) : f[x];
      if (owner != nullptr && lane == 0) owner[row] = (int)i;
      if (start_out != nullptr && lane == 0) start_out[row] = st;
    }
  }
}

/* csgpu_many_fold_halvings: halvings[owner[t]] += sub_halvings[t] for every t < total with owner[t] >= 0, one relaxed
 * agent-scope 64-bit add each; shaped like cs_dive_fold */
__global__ __launch_bounds__(256) void cs_walk_fold_halvings(const long long *__restrict__ sub_halvings,
                                                             const int *__restrict__ owner, long long total,
                                                             long long *halvings) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int o = owner[t];
  if (o < 0) return;
  const long long h = sub_halvings[t];
  if (h != 0) __hip_atomic_fetch_add(halvings + o, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ---- clause models past 512 clauses: the records in LDS (csgpu_solve_many_clauses_wide; CS_WALK_WIDE of
 * cs_walk_body.hip.h, the rounds of cs_rounds_wide_body.hip.h).  cs_walk_clauses's walk and arguments; the dynamic LDS is
 * the staged block, 16 (T.n_clauses + T.n_lits) bytes, and behind it the slices of the workgroup's waves */
template <bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_wide(cs_tables T, cs_walk_io io) {
#define CS_WALK_CK 0
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 0
#define CS_WALK_ORDER 0
#define CS_WALK_WIDE 1
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

/* the same with cs_walk_resume's checkpoints and arguments (csgpu_solve_many_clauses_wide_checkpointed / _wide_resume): the
 * slot layout, the header, CS_WALK_CK_MAGIC and the objective code are cs_walk_resume's */
template <bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_wide_resume(cs_tables T, cs_walk_io io, cs_walk_ck ck) {
#define CS_WALK_CK 1
#define CS_WALK_UPTO 0
#define CS_WALK_RESTART 0
#define CS_WALK_STREAM 0
#define CS_WALK_FROM 0
#define CS_WALK_ORDER 0
#define CS_WALK_WIDE 1
#include "cs_walk_body.hip.h"
#undef CS_WALK_WIDE
#undef CS_WALK_ORDER
#undef CS_WALK_FROM
#undef CS_WALK_STREAM
#undef CS_WALK_RESTART
#undef CS_WALK_UPTO
#undef CS_WALK_CK
}

/* csgpu_many_fold_best: every sub-record with a solution offers (rank(best) << 32) | row to its owner's key, one relaxed
 * agent-scope 64-bit unsigned min; the caller set the keys to all ones.  total < 2^32 (the host checks it) */
__global__ __launch_bounds__(256) void cs_walk_fold_best(const cs_dive_result *__restrict__ sub, const int *__restrict__ best,
                                                         const int *__restrict__ owner, long long total, int sense,
                                                         unsigned long long *__restrict__ key) {
  const long long t = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
  if (t >= total) return;
  const int o = owner[t];
  if (o < 0 || sub[t].solutions <= 0) return;
  __hip_atomic_fetch_min(key + o, (unsigned long long)cs_many_best_key(sense, best[t], (uint32_t)t), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

#endif
