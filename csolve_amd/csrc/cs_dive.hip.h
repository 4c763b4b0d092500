/* cs_dive.hip.h -- cs_dive_shave: many instances of ONE model in one launch, a whole depth-first search per wavefront.
 *
 * For the models of kernel 7 (cs_shave.hip.h: pure binary-!= networks of at most 256 variables whose dense pair table
 * fits LDS).  An instance is a row of root domains inside the model's own; a wave draws an instance number, runs the
 * instance's root node (a `var < 0` node: every valued variable pushes), and then walks the instance's tree by itself
 * -- the reference's solve() (csolve.c:398-476) once per wavefront:
 *
 *   branch    the open variable with the smallest interval, ties to the lowest index: the wave minimum of
 *             (width - 1) << 8 | index, as in cs_step_shave; values in ascending order
 *   child     x = value on the current node's registers, then cs_shave_core::fixpoint.  Every value runs its fixpoint:
 *             a value that a valued neighbour forbids fails in its first PUSH (the neighbour's bounds cross), which is
 *             the node and the cut cs_step_shave counts for it without launching it
 *   descend   a consistent child with open variables becomes the current node; unless the value was the node's last,
 *             the node is pushed: one frame = its row (n intervals relative to the root lower bounds) and one more
 *             8-byte entry {branching variable, next value}, written and read back by lane 0
 *   solution  a consistent child without open variables (on a != network nothing else has to be evaluated)
 *   pop       when the current node's values are used up; an empty stack ends the instance
 *
 * The stack is the wave's slice of a workspace in device memory, `frames` frames of n + 1 entries: a push needs a child
 * with an open variable, every level values at least one variable, so at most n - 1 frames are ever in use (the kernel
 * checks all the same and reports CSGPU_MANY_LIMIT rather than write past its slice).  A lane reads back only what it
 * wrote itself: no fence, no __syncthreads() after the table is in LDS, no atomic per node.
 *
 * Counters per instance, with cs_step_shave's meanings: nodes = children tried, cuts = inconsistent children, props =
 * narrowings of the consistent children (every bound move is one; the assignment itself is none), solutions; root_props
 * = narrowings of the root node (0 when it is inconsistent).  max_nodes is checked before a child is tried: an instance
 * that would need one more stops with exactly max_nodes.
 *
 * Work distribution: persistent waves, one instance per ticket.  Instance i belongs to shard i mod S (S = min(grid,
 * CS_DIVE_SHARDS) counters, each on its own 64-byte line), workgroup b draws from shard b mod S, and every wave stops
 * at its first ticket past the end.  A launch therefore draws exactly (instances of the shard + waves of the shard)
 * tickets per counter, and the wave that draws the last of them writes the counter back to zero: nothing is cleared
 * between launches, back-to-back launches on one stream need no host in between.
 *
 * Checkpoints (cs_dive_resume, csgpu_solve_many_checkpointed / _resume): the same loop -- both kernels include
 * cs_dive_body.hip.h, with CS_DIVE_CK 0 and 1.  An instance that stops at max_nodes with work left draws a slot of a
 * pool (one relaxed atomic add by lane 0) and leaves there what the loop needs to go on at "try value nv of variable bv
 * on the node plo / phi":
 *
 *   slot = n + 1 frames of n + 1 entries (8 bytes each)
 *   frame 0       the header: entry 0 = {depth, CS_DIVE_CK_MAGIC}, written and read by lane 0
 *   frame 1 + d   stack frame d (d < depth), exactly as in the workspace
 *   frame 1 + depth   the current node: its row and {bv, nv}
 *
 * The counters (props reduced over the wave) go to the instance's result record as always and are read back from
 * there; xlo / bhi are those of variable bv in the current node's row and are read from it again.  A resumed instance
 * uses the frames of its slot AS its stack: the slot stays with the instance until the pool is reset, so a slice after
 * the first copies nothing in and, when it stops again, writes only the current node; it needs no workspace at all.  A
 * fresh instance walks in the wave's workspace slice and copies its depth frames out when it stops (every lane copies
 * the entries it wrote itself).  The budget of a resumed instance counts the nodes of this launch; everything else
 * accumulates, so a walk in slices gives, counter for counter, the walk with the summed budget.
 *
 * Up to k solutions (cs_dive_upto, csgpu_solve_many_upto / _upto_checkpointed / _upto_resume): the same loop a third
 * time, with CS_DIVE_CK 1 and CS_DIVE_UPTO 1.  The instance walks the ALL walk and leaves right after its k-th solution,
 * as ANY leaves after its first; solution j goes to row j of the instance's k rows ([count][k][n], the index in 64 bits).
 * k and the row index are scalars.  The kernel is checkpoint-capable and serves all three entries: the plain call
 * passes a pool of capacity 0, which the kernel then never touches.  A resumed instance whose record already counts k
 * solutions (k is per call) ends DONE before it tries a node: only so the row index stays below k.
 *
 * Restarts (cs_dive_restart, csgpu_solve_many_restarts): the same loop a fourth time, CS_DIVE_CK 0 and CS_DIVE_RESTART 1,
 * ANY only and without checkpoints.  The deep walks of a batch are the heavy tail of a depth-first search with a fixed
 * value order; the reference cures it with Luby restarts and a seeded value order (csolve.c:76-83, 264-276, 331-338).
 * Here a node tries its values in a rotation of the ascending order that depends on (seed of the instance, run,
 * variable), cs_many_start / cs_many_rotated of cs_arith.h, and after more than threshold x restart_base failed children
 * the walk starts again from the root node's fixpoint with run + 1 and the next Luby threshold.  Counters and the budget
 * run over all runs; a restart costs no node.  The root fixpoint is kept in the wave's n-th frame, which the walk never
 * uses.  Everything new is a scalar.
 *
 * Every solution (cs_dive_stream, csgpu_solve_many_stream): the same loop a fifth time, CS_DIVE_CK 1 and CS_DIVE_STREAM 1,
 * the ALL walk only.  A solution is appended to one output stream shared by all waves: lane 0 adds 1 to one 64-bit word
 * (relaxed, agent scope), the old value is the row -- every lane stores its variables there, lane 0 the owner -- unless it
 * is past the capacity: then the child is NOT counted and the instance stops with CSGPU_MANY_FULL and a checkpoint that
 * stands before that very value, so the next call tries it again.  The fixpoint runs on copies, the parent node is intact.
 * Whether an instance is fresh or goes on from a slot is a fact per instance here (slots[i] == -2 or >= 0): a fresh one
 * walks in the wave's workspace slice and copies its frames out when it stops, a resumed one walks in its slot.  A wave
 * that finds the stream full when it has drawn a ticket does not walk.  New per-wave state is scalars.
 *
 * The allowed walk in slices and spread (cs_dive_allowed_resume / cs_dive_allowed_upto_resume, cs_dive_allowed_children /
 * cs_dive_allowed_fanout; csgpu_solve_many_allowed_checkpointed / _resume and the up-to-k pair, csgpu_many_allowed_
 * checkpoint_children / _fanout): cs_dive_allowed_body.hip.h with CS_DIVE_CK 1.  The slot layout is cs_dive_resume's: a
 * frame of the allowed walk is {row, bv, next = value + 1} already, and coming back to a frame the kernel rebuilds
 * allowed(bv) on the frame's row and drops the bits below next -- exactly what a resume does on the current node, whose
 * entry is {bv, nv} with nv the lowest bit still in aw (the budget is compared after the pop loop: aw is not empty).  The
 * header's magic is CS_DIVE_CK_MAGIC_ALLOWED: the trees and counters of the two walks differ, so each walk's kernels refuse
 * the other's slots before they read them; cs_dive_export takes both ([next, hi] covers the open subtrees of either walk).
 * The spread lists, per frame, only the untried values that no valued variable of the frame's row forbids, from the dense
 * table in global memory, and folds with cs_dive_fold.  Exact because the allowed sets are a function of the node's row and
 * the table only and the fixpoint of a != network is unique: the root node of a child row is the child's fixpoint, the
 * sub-walk the subtree (the argument stands with the kernels below and in csolve_gpu.h).
 * Resources (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / SGPRs / scratch bytes / waves per SIMD; 8- and 16-bit
 * table entries give the same figures):
 *                                 R=1 NW=1      R=1 NW=4      R=2 NW=1      R=2 NW=4      R=4 NW=1       R=4 NW=4
 *   cs_dive_allowed_resume        46/78/0/8     47/78/0/8     54/78/0/8     64/78/0/8     79/106/0/6     99/106/0/4
 *   cs_dive_allowed_upto_resume   42/78/0/8     43/78/0/8     53/78/0/8     64/78/0/8     78/106/0/6     98/106/0/4
 *   cs_dive_allowed_children<E> 29/49/0/8, cs_dive_allowed_fanout<E> 29/68/0/8.  New per-wave state across the child's
 *   fixpoint is scalars (slot, kept, depth0, nodes0, resumed). */
#ifndef CS_DIVE_HIP_H
#define CS_DIVE_HIP_H

#include "cs_shave.hip.h"
#include "cs_step.hip.h"

#define CS_DIVE_SHARDS 64
#define CS_DIVE_TICKET_STRIDE 16 /* unsigned words between two counters */

/* csgpu_many_result (csolve_gpu.h) */
struct cs_dive_result {
  int status, root_props;
  long long nodes, cuts, props, solutions;
};

/* a value every lane loaded from the same address, as the scalar it is */
static __device__ __forceinline__ long long cs_dive_uniform(long long x) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)x);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)x >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

struct cs_dive_io {
  const cs_val *roots;     /* [count][n] */
  int count;
  int all;                 /* 0: stop at the first solution, 1: walk the whole tree (cs_dive_upto does not read it) */
  long long max_nodes;
  cs_dive_result *results; /* [count] */
  int *solutions;          /* [count][n] or NULL: the first solution of an instance that has one; cs_dive_upto:
                              [count][k][n] or NULL, the first k in walk order */
  cs_val *stack;           /* [waves][frames][n + 1] */
  int frames;
  unsigned *tickets;       /* CS_DIVE_SHARDS counters, zero between launches */
};

#define CS_DIVE_CK_MAGIC 0x636b7074 /* header entry 0 .hi of a slot that holds a checkpoint */
#define CS_DIVE_CK_MAGIC_ALLOWED 0x636b616c /* the same of a slot written by the allowed walk: another tree, other counters */

/* the checkpoint pool and the slot numbers of a call (cs_dive_resume) */
struct cs_dive_ck {
  cs_val *pool;              /* [capacity][n + 1][n + 1] */
  unsigned long long *next;  /* slots handed out since the last reset (it counts on past capacity) */
  int capacity;              /* cs_dive_upto: 0 = no pool (pool, next and slots are not touched) */
  int resume;                /* 0: fresh instances from io.roots; 1: instance i goes on from slot slots[i] */
  int *slots;                /* [count]: the slot of an instance stopped with a checkpoint, else -1 */
};

/* the restart walk of a call (cs_dive_restart) */
struct cs_dive_rs {
  const unsigned *seeds;  /* [count], or NULL: `seed` for every instance */
  int *restarts;          /* [count] or NULL: the restarts of an instance, written by lane 0 with its record */
  long long restart_base; /* a run ends after more than threshold x base failures (Luby thresholds); 0: no restarts */
  unsigned seed;
  int flags;              /* bit 0: CSGPU_MANY_ROTATE_FIRST, run 0 rotates as well */
};

/* the solution stream of a call (cs_dive_stream): csgpu_many_stream */
struct cs_dive_out {
  int *rows;                 /* [capacity][n] */
  int *owner;                /* [capacity] */
  unsigned long long *count; /* append attempts since the caller zeroed it: the kernel only adds */
  long long capacity;        /* >= 1 */
};

template <typename E, int R>
__global__ __launch_bounds__(1024, (R <= 2 ? 8 : 4)) void cs_dive_shave(int n, const E *__restrict__ tab_g, int slots, int dmin,
                                                                        const int *__restrict__ root_lo,
                                                                        const int *__restrict__ root_hi,
                                                                        const int *__restrict__ sym_off, size_t tab_bytes,
                                                                        cs_dive_io io) {
#define CS_DIVE_CK 0
#define CS_DIVE_UPTO 0
#define CS_DIVE_RESTART 0
#define CS_DIVE_STREAM 0
#include "cs_dive_body.hip.h"
#undef CS_DIVE_STREAM
#undef CS_DIVE_RESTART
#undef CS_DIVE_UPTO
#undef CS_DIVE_CK
}

/* the same with checkpoints: fresh instances (ck.resume == 0) or the instances of ck.slots going on */
template <typename E, int R>
__global__ __launch_bounds__(1024, (R <= 2 ? 8 : 4)) void cs_dive_resume(int n, const E *__restrict__ tab_g, int slots, int dmin,
                                                                         const int *__restrict__ root_lo,
                                                                         const int *__restrict__ root_hi,
                                                                         const int *__restrict__ sym_off, size_t tab_bytes,
                                                                         cs_dive_io io, cs_dive_ck ck) {
#define CS_DIVE_CK 1
#define CS_DIVE_UPTO 0
#define CS_DIVE_RESTART 0
#define CS_DIVE_STREAM 0
#include "cs_dive_body.hip.h"
#undef CS_DIVE_STREAM
#undef CS_DIVE_RESTART
#undef CS_DIVE_UPTO
#undef CS_DIVE_CK
}

/* the same again, leaving an instance right after its `upto`-th solution and keeping all of them (upto >= 1) */
template <typename E, int R>
__global__ __launch_bounds__(1024, (R <= 2 ? 8 : 4)) void cs_dive_upto(int n, const E *__restrict__ tab_g, int slots, int dmin,
                                                                       const int *__restrict__ root_lo,
                                                                       const int *__restrict__ root_hi,
                                                                       const int *__restrict__ sym_off, size_t tab_bytes,
                                                                       cs_dive_io io, cs_dive_ck ck, int upto) {
#define CS_DIVE_CK 1
#define CS_DIVE_UPTO 1
#define CS_DIVE_RESTART 0
#define CS_DIVE_STREAM 0
#include "cs_dive_body.hip.h"
#undef CS_DIVE_STREAM
#undef CS_DIVE_RESTART
#undef CS_DIVE_UPTO
#undef CS_DIVE_CK
}

/* the ANY walk with a seeded rotation of every node's value order and Luby restarts (csgpu_solve_many_restarts); io.all
 * is 0 */
template <typename E, int R>
__global__ __launch_bounds__(1024, (R <= 2 ? 8 : 4)) void cs_dive_restart(int n, const E *__restrict__ tab_g, int slots, int dmin,
                                                                          const int *__restrict__ root_lo,
                                                                          const int *__restrict__ root_hi,
                                                                          const int *__restrict__ sym_off, size_t tab_bytes,
                                                                          cs_dive_io io, cs_dive_rs rs) {
#define CS_DIVE_CK 0
#define CS_DIVE_UPTO 0
#define CS_DIVE_RESTART 1
#define CS_DIVE_STREAM 0
#include "cs_dive_body.hip.h"
#undef CS_DIVE_STREAM
#undef CS_DIVE_RESTART
#undef CS_DIVE_UPTO
#undef CS_DIVE_CK
}

/* the ALL walk that appends every solution to `out` and steps back when there is no room; ck.resume and io.all are not
 * read: ck.slots[i] says per instance whether it starts (-2), goes on (>= 0) or is finished (anything else) */
template <typename E, int R>
__global__ __launch_bounds__(1024, (R <= 2 ? 8 : 4)) void cs_dive_stream(int n, const E *__restrict__ tab_g, int slots, int dmin,
                                                                         const int *__restrict__ root_lo,
                                                                         const int *__restrict__ root_hi,
                                                                         const int *__restrict__ sym_off, size_t tab_bytes,
                                                                         cs_dive_io io, cs_dive_ck ck, cs_dive_out out) {
#define CS_DIVE_CK 1
#define CS_DIVE_UPTO 0
#define CS_DIVE_RESTART 0
#define CS_DIVE_STREAM 1
#include "cs_dive_body.hip.h"
#undef CS_DIVE_STREAM
#undef CS_DIVE_RESTART
#undef CS_DIVE_UPTO
#undef CS_DIVE_CK
}

/* ---- branching on the allowed values (cs_dive_allowed, cs_dive_allowed_upto: csgpu_solve_many_allowed / _allowed_upto)
 *
 * The walk of cs_dive_shave with another branching rule (specified in csolve_gpu.h): at a node, a value of an open variable
 * that some VALUED variable forbids through a clause of the model is neither tried nor counted; the walk branches on the
 * open variable with the fewest other ("allowed") values and tries those in ascending order.  On a != network an interval
 * hides holes, and the width says little about how constrained a variable is.
 *
 * Allowed sets: NW 32-bit words per variable, bit k = the value root_lo + k, the coordinates of the node's bounds.  They
 * are REBUILT from the node's row whenever a node is entered or a frame is popped, and are dead before the child's
 * fixpoint starts: frames, slots and the workspace hold nothing new.  For every valued variable u, lane w reads its own
 * entries of u's table row -- the conflict-free LDS read of cs_shave_core::push_var, f = cd - row[k * W + r2 * CS_WAVE],
 * the sentinel giving f < 0 -- and sets bit f of its forbidden words: (valued variables x slots x R) LDS reads per ENTERED
 * node, no atomics, no lane reads what another wrote.  32-bit words: the library contains no 64-bit vector shift by a
 * register amount.  NW is 1 (root widths up to 32) or 4 (up to 128); wider models are refused. */

/* al[r][j] = the allowed values of the variable (lane, r) in the node plo / phi, valued variables pval: the values of
 * [plo, phi] that no valued variable forbids (meaningful for open variables only) */
template <typename E, int R, int NW>
__device__ __forceinline__ void cs_dive_allowed_sets(const cs_shave_core<E, R, 0, false> &C, const int (&plo)[R],
                                                     const int (&phi)[R], const unsigned long long (&pval)[R],
                                                     unsigned (&al)[R][NW]) {
  constexpr int W = CS_WAVE * R;
  unsigned fb[R][NW];
#pragma unroll
  for (int r2 = 0; r2 < R; r2++)
#pragma unroll
    for (int j = 0; j < NW; j++) fb[r2][j] = 0u;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int cdv = plo[r] + C.kb[r]; /* value - dmin of a valued variable */
    unsigned long long bits = pval[r];
    while (bits != 0ull) {
      const int ul = __builtin_ctzll(bits);
      bits = cs_bitset0(bits, ul);
      const int cd = __builtin_amdgcn_readlane(cdv, ul);
      const E *row = C.s_tab + (size_t)(ul + r * CS_WAVE) * C.slots * W + C.lane;
      for (int k = 0; k < C.slots; k++) {
#pragma unroll
        for (int r2 = 0; r2 < R; r2++) {
          const int f = cd - (int)row[k * W + r2 * CS_WAVE]; /* the value of w that u forbids (sentinel: < 0) */
          const unsigned bit = 1u << (f & 31);
          if (NW == 1) {
            fb[r2][0] |= (unsigned)f < 32u ? bit : 0u;
          } else {
            const int word = f >> 5; /* negative for the sentinel */
#pragma unroll
            for (int j = 0; j < NW; j++) fb[r2][j] |= word == j ? bit : 0u;
          }
        }
      }
    }
  }
#pragma unroll
  for (int r2 = 0; r2 < R; r2++) {
#pragma unroll
    for (int j = 0; j < NW; j++) {
      const int lo = plo[r2] - 32 * j, hi = phi[r2] - 32 * j; /* the bounds in word j's coordinates */
      const unsigned range = (0xffffffffu >> (31 - (hi > 31 ? 31 : hi & 31))) & (0xffffffffu << (lo < 0 ? 0 : lo & 31));
      al[r2][j] = hi < 0 || lo > 31 ? 0u : ~fb[r2][j] & range;
    }
  }
}

/* NW wave-uniform words of values still to be tried: is one left; the lowest, which is taken out; those below `next` out */
template <int NW>
__device__ __forceinline__ bool cs_dive_any_bits(const unsigned (&aw)[NW]) {
  unsigned any = 0u;
#pragma unroll
  for (int j = 0; j < NW; j++) any |= aw[j];
  return any != 0u;
}
template <int NW>
__device__ __forceinline__ int cs_dive_take_lowest(unsigned (&aw)[NW]) {
  int value = 0;
  bool taken = false;
#pragma unroll
  for (int j = 0; j < NW; j++) {
    const bool here = !taken && aw[j] != 0u;
    if (here) {
      value = 32 * j + __builtin_ctz(aw[j]);
      aw[j] &= aw[j] - 1u;
    }
    taken = taken || here;
  }
  return value;
}
template <int NW>
__device__ __forceinline__ void cs_dive_bits_from(unsigned (&aw)[NW], int next) {
#pragma unroll
  for (int j = 0; j < NW; j++) {
    const int t = next - 32 * j;
    aw[j] &= t <= 0 ? 0xffffffffu : (t > 31 ? 0u : 0xffffffffu << t);
  }
}

template <typename E, int R, int NW>
__global__ __launch_bounds__(1024, (R <= 2 ? 8 : 4)) void cs_dive_allowed(int n, const E *__restrict__ tab_g, int slots, int dmin,
                                                                          const int *__restrict__ root_lo,
                                                                          const int *__restrict__ root_hi,
                                                                          const int *__restrict__ sym_off, size_t tab_bytes,
                                                                          cs_dive_io io) {
#define CS_DIVE_CK 0
#define CS_DIVE_UPTO 0
#include "cs_dive_allowed_body.hip.h"
#undef CS_DIVE_UPTO
#undef CS_DIVE_CK
}

/* the same, leaving an instance right after its `upto`-th solution and keeping all of them (upto >= 1; io.all is not read) */
template <typename E, int R, int NW>
__global__ __launch_bounds__(1024, (R <= 2 ? 8 : 4)) void cs_dive_allowed_upto(int n, const E *__restrict__ tab_g, int slots,
                                                                               int dmin, const int *__restrict__ root_lo,
                                                                               const int *__restrict__ root_hi,
                                                                               const int *__restrict__ sym_off, size_t tab_bytes,
                                                                               cs_dive_io io, int upto) {
#define CS_DIVE_CK 0
#define CS_DIVE_UPTO 1
#include "cs_dive_allowed_body.hip.h"
#undef CS_DIVE_UPTO
#undef CS_DIVE_CK
}

/* the allowed walk with checkpoints (csgpu_solve_many_allowed_checkpointed / _resume): fresh instances (ck.resume == 0) or
 * the instances of ck.slots going on.  A slot is laid out as cs_dive_resume's and carries CS_DIVE_CK_MAGIC_ALLOWED: the
 * trees differ, so a slot of one walk is no checkpoint of the other. */
template <typename E, int R, int NW>
__global__ __launch_bounds__(1024, (R <= 2 ? 8 : 4)) void cs_dive_allowed_resume(int n, const E *__restrict__ tab_g, int slots,
                                                                                 int dmin, const int *__restrict__ root_lo,
                                                                                 const int *__restrict__ root_hi,
                                                                                 const int *__restrict__ sym_off, size_t tab_bytes,
                                                                                 cs_dive_io io, cs_dive_ck ck) {
#define CS_DIVE_CK 1
#define CS_DIVE_UPTO 0
#include "cs_dive_allowed_body.hip.h"
#undef CS_DIVE_UPTO
#undef CS_DIVE_CK
}

/* the same up to k (csgpu_solve_many_allowed_upto_checkpointed / _resume); the pool always has slots here: the plain
 * up-to-k call launches cs_dive_allowed_upto */
template <typename E, int R, int NW>
__global__ __launch_bounds__(1024, (R <= 2 ? 8 : 4)) void cs_dive_allowed_upto_resume(int n, const E *__restrict__ tab_g, int slots,
                                                                                      int dmin, const int *__restrict__ root_lo,
                                                                                      const int *__restrict__ root_hi,
                                                                                      const int *__restrict__ sym_off,
                                                                                      size_t tab_bytes, cs_dive_io io, cs_dive_ck ck,
                                                                                      int upto) {
#define CS_DIVE_CK 1
#define CS_DIVE_UPTO 1
#include "cs_dive_allowed_body.hip.h"
#undef CS_DIVE_UPTO
#undef CS_DIVE_CK
}

/* csgpu_many_checkpoint_states: frame d of slot `slot` (d <= depth, the oldest first) as a state in absolute bounds, its
 * branching variable narrowed to the values not tried yet, [next, hi].  One workgroup per frame. */
__global__ void cs_dive_export(int n, const int *__restrict__ root_lo, const cs_val *__restrict__ slot_base,
                               cs_val *__restrict__ states) {
  const size_t fstride = (size_t)n + 1;
  const cs_val *f = slot_base + fstride * (1 + (size_t)blockIdx.x);
  const cs_val meta = f[n];
  for (int v = threadIdx.x; v < n; v += blockDim.x) {
    cs_val d = f[v];
    if (v == meta.lo) d.lo = meta.hi;
    states[(size_t)blockIdx.x * n + v] = cs_interval(d.lo + root_lo[v], d.hi + root_lo[v]);
  }
}

/* ---- a stopped ALL walk spread over the waves of the next launch (csgpu_many_checkpoint_children / _fanout, csgpu_many_fold)
 *
 * A checkpoint is a list of frames "node, branching variable bv, next value": the untried children of the walk are, in walk
 * order, the values next .. node[bv].hi of the current node (frame `depth`), then those of frame depth - 1, down to frame
 * 0.  Child (d, v) walked as a root row of its own -- the node in absolute bounds with bv = [v, v] -- gives its owner
 * exactly what the one walk counts for that child and everything below it:
 *
 *   nodes     1 + sub.nodes
 *   cuts      sub.cuts, plus 1 if the row was inconsistent as a root (DONE, no node, no solution)
 *   props     sub.root_props + sub.props   (the fixpoint of a != network is unique, props counts units shaved, and the
 *                                           assignment itself is counted on neither side)
 *   solutions sub.solutions
 *
 * The kernels are not templated: a slot is 8-byte entries relative to the root lower bounds whatever E and R wrote it.
 * One wave per instance, 64-bit row indices, no atomics in the count or the fan-out; the fold adds with relaxed
 * agent-scope 64-bit atomics.  A slot is checked before anything that depends on it is read: a slot number outside the
 * pool, a header without the magic, a depth outside [0, n), a frame whose bv is outside [0, n), whose node's bounds of bv
 * are outside the root domain's width or whose next value is outside those bounds give -1, never a count. */
#define CS_DIVE_FAN_WAVES 4 /* instances per workgroup */

static __device__ __forceinline__ long long cs_dive_slot_children(int n, const int *__restrict__ root_lo,
                                                                  const int *__restrict__ root_hi,
                                                                  const cs_val *__restrict__ pool, int capacity, int slot,
                                                                  int lane) {
  if (slot < 0) return 0;
  if (slot >= capacity) return -1;
  const size_t fstride = (size_t)n + 1;
  const cs_val *base = pool + (size_t)slot * (fstride * fstride);
  const cs_val head = base[0];
  const int depth = __builtin_amdgcn_readfirstlane(head.lo);
  if (__builtin_amdgcn_readfirstlane(head.hi) != CS_DIVE_CK_MAGIC || depth < 0 || depth >= n) return -1;
  long long mine = 0;
  bool bad = false;
  for (int d = lane; d <= depth && !bad; d += CS_WAVE) {
    const cs_val *f = base + fstride * (1 + (size_t)d);
    const cs_val meta = f[n];
    if (meta.lo < 0 || meta.lo >= n) {
      bad = true;
    } else {
      const cs_val node = f[meta.lo];
      if (node.lo < 0 || node.hi > root_hi[meta.lo] - root_lo[meta.lo] || meta.hi < node.lo || meta.hi > node.hi)
        bad = true;
      else
        mine += (long long)node.hi - (long long)meta.hi + 1;
    }
  }
  if (__ballot(bad) != 0ull) return -1;
  for (int o = CS_WAVE / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o, CS_WAVE);
  return cs_dive_uniform(mine);
}

/* children[i] = the untried children of the checkpoint in slot slots[i]: 0 for slots[i] < 0, -1 for a slot that is refused */
__global__ __launch_bounds__(CS_DIVE_FAN_WAVES * CS_WAVE) void cs_dive_children(int n, const int *__restrict__ root_lo,
                                                                                const int *__restrict__ root_hi,
                                                                                const cs_val *__restrict__ pool, int capacity,
                                                                                const int *__restrict__ slots, long long count,
                                                                                long long *__restrict__ children) {
  const int lane = (int)(threadIdx.x % CS_WAVE);
  const long long i = (long long)blockIdx.x * CS_DIVE_FAN_WAVES + (long long)(threadIdx.x / CS_WAVE);
  if (i >= count) return;
  const int slot = __builtin_amdgcn_readfirstlane(slots[i]);
  const long long c = cs_dive_slot_children(n, root_lo, root_hi, pool, capacity, slot, lane);
  if (lane == 0) children[i] = c;
}

/* rows[offsets[i] ..] = the children of instance i in walk order, owner[row] = i.  The instance is counted again first: it
 * writes nothing unless offsets[i + 1] - offsets[i] is its count and its rows lie inside [0, total) */
__global__ __launch_bounds__(CS_DIVE_FAN_WAVES * CS_WAVE) void cs_dive_fanout(int n, const int *__restrict__ root_lo,
                                                                              const int *__restrict__ root_hi,
                                                                              const cs_val *__restrict__ pool, int capacity,
                                                                              const int *__restrict__ slots, long long count,
                                                                              const long long *__restrict__ offsets,
                                                                              long long total, cs_val *__restrict__ rows,
                                                                              int *__restrict__ owner) {
  const int lane = (int)(threadIdx.x % CS_WAVE);
  const long long i = (long long)blockIdx.x * CS_DIVE_FAN_WAVES + (long long)(threadIdx.x / CS_WAVE);
  if (i >= count) return;
  const int slot = __builtin_amdgcn_readfirstlane(slots[i]);
  if (slot < 0) return;
  const long long mine = cs_dive_slot_children(n, root_lo, root_hi, pool, capacity, slot, lane);
  const long long off = cs_dive_uniform(offsets[i]), end = cs_dive_uniform(offsets[i + 1]);
  if (mine <= 0 || off < 0 || end > total || end - off != mine) return;
  const size_t fstride = (size_t)n + 1;
  const cs_val *base = pool + (size_t)slot * (fstride * fstride);
  const int depth = __builtin_amdgcn_readfirstlane(base[0].lo);
  long long row = off;
  for (int d = depth; d >= 0; d--) {
    const cs_val *f = base + fstride * (1 + (size_t)d);
    const cs_val meta = f[n];
    const int bv = __builtin_amdgcn_readfirstlane(meta.lo);
    const int next = __builtin_amdgcn_readfirstlane(meta.hi);
    const int hi = __builtin_amdgcn_readfirstlane(f[bv].hi);
    for (long long v = next; v <= (long long)hi && row < end; v++, row++) {
      cs_val *dst = rows + (size_t)row * (size_t)n;
      for (int x = lane; x < n; x += CS_WAVE) {
        const cs_val e = f[x];
        const int b = root_lo[x];
        dst[x] = x == bv ? cs_interval((int)v + b, (int)v + b) : cs_interval(e.lo + b, e.hi + b);
      }
      if (owner != nullptr && lane == 0) owner[row] = (int)i;
    }
  }
}

/* results[owner[t]] += the contribution of sub-instance record t (above); status and root_props of the owner stay */
__global__ __launch_bounds__(256) void cs_dive_fold(const cs_dive_result *__restrict__ sub, const int *__restrict__ owner,
                                                    long long total, cs_dive_result *results) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int o = owner[t];
  if (o < 0) return;
  const cs_dive_result r = sub[t];
  cs_dive_result *dst = results + o;
  const long long cuts = r.cuts + (r.status == 0 /* CSGPU_MANY_DONE */ && r.nodes == 0 && r.solutions == 0 ? 1 : 0);
  const long long props = (long long)r.root_props + r.props;
  __hip_atomic_fetch_add(&dst->nodes, 1 + r.nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (cuts != 0) __hip_atomic_fetch_add(&dst->cuts, cuts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (props != 0) __hip_atomic_fetch_add(&dst->props, props, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (r.solutions != 0) __hip_atomic_fetch_add(&dst->solutions, r.solutions, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ---- the same for a stopped ALLOWED walk (csgpu_many_allowed_checkpoint_children / _fanout; the fold is cs_dive_fold)
 *
 * The untried children of frame d of an allowed slot are the values c of [next, node[bv].hi] that no valued variable of the
 * frame's row forbids, ascending; frames from `depth` down to 0, as above.  The forbidden values of the ONE variable bv come
 * from the model's dense pair table in global memory, with the arithmetic of cs_dive_allowed_sets: for a valued u and slot k,
 * f = value(u) + kb(u) - tab[(u * slots + k) * W + bv], the sentinel giving f < 0.  Lanes stride over u, an OR across the wave
 * gives the four words.  A cold path: no LDS, table reads from global memory.
 *
 * The split is exact for the reason it is exact on the width walk.  The allowed sets are a function of the node's row and
 * the table only, so a child row -- the frame's row with bv = [c, c] -- names its subtree whoever walks it; the fixpoint of a
 * != network is unique, so the root node of the child row IS the child's fixpoint and the sub-walk branches as the one walk
 * does below it.  Hence, per child: nodes 1 + sub.nodes; cuts sub.cuts + (inconsistent as a root); props sub.root_props +
 * sub.props; solutions sub.solutions -- cs_dive_fold's sums.  A value that a valued variable forbids is no child: the walk
 * neither tries nor counts it, and as a root row it would be one more cut.
 *
 * The slot checks are cs_dive_slot_children's, each compared before what depends on it is read, with the other magic; a
 * node whose bounds of bv pass the 128 values the sets hold is refused too.  One wave per instance, CS_DIVE_FAN_WAVES
 * instances per workgroup, 64-bit row indices, no atomics.  Templated on the table's entry type alone. */
#define CS_DIVE_ALLOWED_WORDS 4 /* 32-bit words of allowed values: 128, the widest root domain of the allowed walk */

/* aw = the untried allowed values of the frame f (wave-uniform), bv its branching variable; false: the frame is refused */
template <typename E>
static __device__ __forceinline__ bool cs_dive_allowed_frame(int n, const int *__restrict__ root_lo,
                                                             const int *__restrict__ root_hi, const E *__restrict__ tab_g,
                                                             int slots, int dmin, int cols, const cs_val *__restrict__ f, int lane,
                                                             unsigned (&aw)[CS_DIVE_ALLOWED_WORDS], int &bv) {
  const cs_val meta = f[n];
  bv = __builtin_amdgcn_readfirstlane(meta.lo);
  const int next = __builtin_amdgcn_readfirstlane(meta.hi);
  if (bv < 0 || bv >= n) return false;
  const cs_val node = f[bv];
  const int lo = __builtin_amdgcn_readfirstlane(node.lo), hi = __builtin_amdgcn_readfirstlane(node.hi);
  if (lo < 0 || hi > root_hi[bv] - root_lo[bv] || hi >= 32 * CS_DIVE_ALLOWED_WORDS || next < lo || next > hi) return false;
  unsigned fb[CS_DIVE_ALLOWED_WORDS];
#pragma unroll
  for (int j = 0; j < CS_DIVE_ALLOWED_WORDS; j++) fb[j] = 0u;
  for (int u = lane; u < n; u += CS_WAVE) {
    const cs_val e = f[u];
    if (e.lo != e.hi) continue; /* an open variable forbids nothing */
    const int cd = e.lo + root_lo[u] - dmin;
    const E *row = tab_g + (size_t)u * (size_t)slots * (size_t)cols + (size_t)bv;
    for (int k = 0; k < slots; k++) {
      const int fv = cd - (int)row[(size_t)k * (size_t)cols]; /* the value of bv that u forbids (sentinel: < 0) */
      const unsigned bit = 1u << (fv & 31);
      const int word = fv >> 5;
#pragma unroll
      for (int j = 0; j < CS_DIVE_ALLOWED_WORDS; j++) fb[j] |= word == j ? bit : 0u;
    }
  }
#pragma unroll
  for (int j = 0; j < CS_DIVE_ALLOWED_WORDS; j++) {
    for (int o = CS_WAVE / 2; o > 0; o >>= 1) fb[j] |= (unsigned)__shfl_xor((int)fb[j], o, CS_WAVE);
    const int l = next - 32 * j, h = hi - 32 * j; /* [next, hi] in word j's coordinates */
    const unsigned range = (0xffffffffu >> (31 - (h > 31 ? 31 : h & 31))) & (0xffffffffu << (l < 0 ? 0 : l & 31));
    aw[j] = (unsigned)__builtin_amdgcn_readfirstlane((int)(h < 0 || l > 31 ? 0u : ~fb[j] & range));
  }
  return true;
}

/* the untried children of the allowed checkpoint in `slot`: 0 for slot < 0, -1 for a slot that is refused */
template <typename E>
static __device__ __forceinline__ long long cs_dive_allowed_slot_children(int n, const int *__restrict__ root_lo,
                                                                          const int *__restrict__ root_hi,
                                                                          const E *__restrict__ tab_g, int slots, int dmin, int cols,
                                                                          const cs_val *__restrict__ pool, int capacity, int slot,
                                                                          int lane) {
  if (slot < 0) return 0;
  if (slot >= capacity) return -1;
  const size_t fstride = (size_t)n + 1;
  const cs_val *base = pool + (size_t)slot * (fstride * fstride);
  const cs_val head = base[0];
  const int depth = __builtin_amdgcn_readfirstlane(head.lo);
  if (__builtin_amdgcn_readfirstlane(head.hi) != CS_DIVE_CK_MAGIC_ALLOWED || depth < 0 || depth >= n) return -1;
  long long count = 0;
  for (int d = depth; d >= 0; d--) {
    unsigned aw[CS_DIVE_ALLOWED_WORDS];
    int bv;
    if (!cs_dive_allowed_frame<E>(n, root_lo, root_hi, tab_g, slots, dmin, cols, base + fstride * (1 + (size_t)d), lane, aw, bv))
      return -1;
#pragma unroll
    for (int j = 0; j < CS_DIVE_ALLOWED_WORDS; j++) count += __popc(aw[j]);
  }
  return count;
}

template <typename E>
__global__ __launch_bounds__(CS_DIVE_FAN_WAVES * CS_WAVE) void cs_dive_allowed_children(
    int n, const int *__restrict__ root_lo, const int *__restrict__ root_hi, const E *__restrict__ tab_g, int slots, int dmin,
    int cols, const cs_val *__restrict__ pool, int capacity, const int *__restrict__ slot_of, long long count,
    long long *__restrict__ children) {
  const int lane = (int)(threadIdx.x % CS_WAVE);
  const long long i = (long long)blockIdx.x * CS_DIVE_FAN_WAVES + (long long)(threadIdx.x / CS_WAVE);
  if (i >= count) return;
  const int slot = __builtin_amdgcn_readfirstlane(slot_of[i]);
  const long long c = cs_dive_allowed_slot_children<E>(n, root_lo, root_hi, tab_g, slots, dmin, cols, pool, capacity, slot, lane);
  if (lane == 0) children[i] = c;
}

/* rows[offsets[i] ..] = the children of instance i in walk order, owner[row] = i.  The instance is counted again first: it
 * writes nothing unless offsets[i + 1] - offsets[i] is its count and its rows lie inside [0, total) */
template <typename E>
__global__ __launch_bounds__(CS_DIVE_FAN_WAVES * CS_WAVE) void cs_dive_allowed_fanout(
    int n, const int *__restrict__ root_lo, const int *__restrict__ root_hi, const E *__restrict__ tab_g, int slots, int dmin,
    int cols, const cs_val *__restrict__ pool, int capacity, const int *__restrict__ slot_of, long long count,
    const long long *__restrict__ offsets, long long total, cs_val *__restrict__ rows, int *__restrict__ owner) {
  const int lane = (int)(threadIdx.x % CS_WAVE);
  const long long i = (long long)blockIdx.x * CS_DIVE_FAN_WAVES + (long long)(threadIdx.x / CS_WAVE);
  if (i >= count) return;
  const int slot = __builtin_amdgcn_readfirstlane(slot_of[i]);
  if (slot < 0) return;
  const long long mine = cs_dive_allowed_slot_children<E>(n, root_lo, root_hi, tab_g, slots, dmin, cols, pool, capacity, slot, lane);
  const long long off = cs_dive_uniform(offsets[i]), end = cs_dive_uniform(offsets[i + 1]);
  if (mine <= 0 || off < 0 || end > total || end - off != mine) return;
  const size_t fstride = (size_t)n + 1;
  const cs_val *base = pool + (size_t)slot * (fstride * fstride);
  const int depth = __builtin_amdgcn_readfirstlane(base[0].lo);
  long long row = off;
  for (int d = depth; d >= 0; d--) {
    const cs_val *f = base + fstride * (1 + (size_t)d);
    unsigned aw[CS_DIVE_ALLOWED_WORDS];
    int bv;
    if (!cs_dive_allowed_frame<E>(n, root_lo, root_hi, tab_g, slots, dmin, cols, f, lane, aw, bv)) return; /* (counted: it passes) */
    while (cs_dive_any_bits<CS_DIVE_ALLOWED_WORDS>(aw) && row < end) {
      const int v = cs_dive_take_lowest<CS_DIVE_ALLOWED_WORDS>(aw);
      cs_val *dst = rows + (size_t)row * (size_t)n;
      for (int x = lane; x < n; x += CS_WAVE) {
        const cs_val e = f[x];
        const int b = root_lo[x];
        dst[x] = x == bv ? cs_interval(v + b, v + b) : cs_interval(e.lo + b, e.hi + b);
      }
      if (owner != nullptr && lane == 0) owner[row] = (int)i;
      row++;
    }
  }
}

#endif
