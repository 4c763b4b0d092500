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
 * atomic. */
#ifndef CS_WALK_HIP_H
#define CS_WALK_HIP_H

#include "cs_kernels.hip.h"
#include "cs_step.hip.h"
#include "cs_dive.hip.h"

struct cs_walk_io {
  const cs_val *roots;     /* [count][n] */
  const cs_val *root_dom;  /* [n]: the model's root domains, which a root row must lie inside */
  int count;
  int all;                 /* 0: leave at the first solution (ANY), 1: walk the whole tree (ALL, MIN, MAX) */
  int sense;               /* cs_objective_bound's: 0 none (ANY / ALL), 1 minimise, 2 maximise */
  int obj_var;             /* "<obj>" under MIN / MAX, else -1 */
  long long max_nodes;
  cs_dive_result *results; /* [count] */
  int *solutions;          /* [count][n] or NULL: the first solution (ANY / ALL), the best one so far (MIN / MAX) */
  int *best;               /* [count] or NULL: MIN / MAX, instances with a solution */
  cs_val *stack;           /* [waves][frames][n + 1] */
  int frames;
  unsigned *tickets;       /* CS_DIVE_SHARDS counters, zero between launches */
};

template <int CPL, bool HAS_TREE>
__global__ __launch_bounds__(CS_BLOCK) void cs_walk_clauses(cs_tables T, cs_walk_io io) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
  const int lane = threadIdx.x & (CS_WAVE - 1);
  const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wave_global = (int)blockIdx.x * CS_WAVES_PER_BLOCK + wave_in_block;
  const int n = T.n_vars;
  const size_t slice_al = ((size_t)n * sizeof(cs_val) + 16 + 15) & ~(size_t)15;
  cs_val *dom = (cs_val *)(cs_lds + wave_in_block * slice_al);
  unsigned *flag = (unsigned *)(dom + n); /* [0]: something changed this round */

  int4 rec[CPL], lit0[CPL], lit1[CPL];
#pragma unroll
  for (int q = 0; q < CPL; q++) {
    const int c = lane + q * CS_WAVE;
    rec[q] = c < T.n_clauses ? T.clause_by_kind[c] : make_int4(CS_CL_SKIP, 0, 0, 0);
    lit0[q] = rec[q].x == CS_CL_OR2 ? T.lit[rec[q].y] : make_int4(0, 0, 0, 0);
    lit1[q] = rec[q].x == CS_CL_OR2 ? T.lit[rec[q].y + 1] : make_int4(0, 0, 0, 0);
  }

  const int nsh = (int)gridDim.x < CS_DIVE_SHARDS ? (int)gridDim.x : CS_DIVE_SHARDS;
  const int shard = (int)(blockIdx.x % nsh);
  const unsigned count_x = io.count > shard ? (unsigned)((io.count - 1 - shard) / nsh + 1) : 0u; /* instances of this shard */
  const unsigned waves_x = (unsigned)((((int)gridDim.x - 1 - shard) / nsh + 1) * CS_WAVES_PER_BLOCK);
  unsigned *my_ticket = io.tickets + (size_t)shard * CS_DIVE_TICKET_STRIDE;
  const size_t fstride = (size_t)n + 1;
  cs_val *const wave_stack = io.stack + (size_t)wave_global * (size_t)io.frames * fstride;

  for (;;) {
    /* the wave meets here before lane 0 draws (cs_dive_body.hip.h: without it the launch never ends) */
    __builtin_amdgcn_wave_barrier();
    unsigned t = 0u;
    if (lane == 0) t = __hip_atomic_fetch_add(my_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    if (t == count_x + waves_x - 1u && lane == 0) __hip_atomic_store(my_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t >= count_x) break;
    const int inst = (int)t * nsh + shard;
    const size_t rrow = (size_t)inst * (size_t)n;

    /* the root row, into the LDS slice */
    bool bad_l = false;
    for (int v = lane; v < n; v += CS_WAVE) {
      const cs_val d = io.roots[rrow + v], r = io.root_dom[v];
      bad_l = bad_l || d.lo > d.hi || d.lo < r.lo || d.hi > r.hi;
      dom[v] = d;
    }
    int status = 0 /* CSGPU_MANY_DONE */, root_props = 0;
    long long nodes = 0, cuts = 0, sols = 0, props = 0; /* scalars */
    int acc_props = 0;                                  /* per lane, added to props every 64 nodes */
    int best = 0;
    bool have_best = false;

    if (__ballot(bad_l) != 0ull) {
      status = 2; /* CSGPU_MANY_BAD_ROOT */
    } else {
      /* One loop for the root node and every child, so that the rounds stand in the kernel once.  `root`: the node in
       * the slice is the root row itself, nothing is assigned and no node is counted.  f: the current node's frame. */
      int depth = 0, bv = 0, nv = 0;
      bool root = true, fresh = true; /* fresh: the slice holds the current node as it was entered */
      cs_val *f = wave_stack;
      for (;;) {
        depth = __builtin_amdgcn_readfirstlane(depth);
        bv = __builtin_amdgcn_readfirstlane(bv);
        nv = __builtin_amdgcn_readfirstlane(nv);
        bool last = false;
        if (!root) {
          if (nodes >= io.max_nodes) { status = 1; /* CSGPU_MANY_LIMIT */ break; }
          if (!fresh) {
            for (int v = lane; v < n; v += CS_WAVE) dom[v] = f[v];
            cs_wave_sync();
          }
          last = nv == __builtin_amdgcn_readfirstlane(dom[bv].hi);
          cs_wave_sync();
          if (lane == 0) {
            dom[bv] = cs_interval(nv, nv); /* the assignment: not counted in PROPS */
            if (have_best) dom[io.obj_var] = cs_objective_bound(io.sense, dom[io.obj_var], best);
          }
        }
        cs_wave_sync();

#include "cs_rounds_body.hip.h"
        (void)rounds;

        /* the open variables of a consistent node, and this lane's candidate for the branching variable */
        int open_vars = 0;
        unsigned kw = 0xffffffffu, kv = 0xffffffffu;
        if (!failed) {
          for (int v0 = 0; v0 < n; v0 += CS_WAVE) { /* uniform trips: the ballot counts every lane */
            const int v = v0 + lane;
            const cs_val d = v < n ? dom[v] : cs_value(0);
            const bool open = d.lo != d.hi;
            const unsigned w = (unsigned)d.hi - (unsigned)d.lo;
            if (open && w < kw) { kw = w; kv = (unsigned)v; }
            open_vars += __popcll(__ballot(open));
          }
        }
        bool descend = false;
        const bool at_root = root;
        if (root) {
          if (failed) break; /* an inconsistent root: DONE, no node, no solution */
          root_props = cs_wave_sum(cx.props);
          root = false;
          descend = open_vars != 0;
        } else {
          nodes++;
          if (failed) {
            cuts++;
          } else {
            acc_props += cx.props; /* consistent children only: kernel 6's props */
            descend = open_vars != 0;
          }
          if ((nodes & 63) == 0) { props += cs_wave_sum(acc_props); acc_props = 0; }
        }
        if (!failed && open_vars == 0) { /* every variable valued: a solution (the root row itself may be the one) */
          sols++;
          if (io.sense != 0) {
            best = __builtin_amdgcn_readfirstlane(dom[io.obj_var].lo);
            have_best = true;
          }
          if ((sols == 1 || io.sense != 0) && io.solutions != nullptr)
            for (int v = lane; v < n; v += CS_WAVE) io.solutions[rrow + v] = dom[v].lo;
          if (!io.all || at_root) break; /* ANY, or the root node was the one solution */
        }
        if (descend) {
          if (!at_root && !last) { /* the parent comes back for its next value */
            if (lane == 0) f[n] = cs_interval(bv, nv + 1);
            depth++;
            f += fstride;
          }
          if (depth >= io.frames) { status = 1; break; } /* cannot happen (frames = n): never write past the slice */
          for (int v = lane; v < n; v += CS_WAVE) f[v] = dom[v];
          const unsigned wmin = cs_wave_min_u32(kw);
          bv = (int)cs_wave_min_u32(kw == wmin ? kv : 0xffffffffu);
          /* cannot happen (an open variable exists): never index past the node */
          if ((unsigned)bv >= (unsigned)n) { status = 1; break; }
          nv = __builtin_amdgcn_readfirstlane(dom[bv].lo);
          fresh = true;
        } else if (last) { /* the node's values are used up */
          if (depth == 0) break;
          depth--;
          f -= fstride;
          cs_val meta = cs_interval(0, 0);
          if (lane == 0) meta = f[n];
          bv = __builtin_amdgcn_readfirstlane(meta.lo);
          nv = __builtin_amdgcn_readfirstlane(meta.hi);
          fresh = false;
        } else {
          nv = nv + 1;
          fresh = false;
        }
      }
    }
    props += cs_wave_sum(acc_props);
    if (lane == 0) {
      cs_dive_result res;
      res.status = status; res.root_props = root_props;
      res.nodes = nodes; res.cuts = cuts; res.props = props; res.solutions = sols;
      io.results[inst] = res;
      if (have_best && io.best != nullptr) io.best[inst] = best;
    }
    cs_wave_sync(); /* the next instance's root row goes into the slice only after every lane has left this one */
  }
}

#endif
