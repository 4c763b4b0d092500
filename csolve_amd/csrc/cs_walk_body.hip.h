/* cs_walk_body.hip.h -- the body of the eleven kernels of cs_walk.hip.h, which includes it inside each of them under seven
 * switches (the seventh, CS_WALK_WIDE, is described at the end of this comment; the fifth, CS_WALK_FROM, is 1 for
 * cs_walk_from -- cs_walk_resume's row, and `start` -- and for
 * cs_walk_order_from; the sixth, CS_WALK_ORDER, for the three cs_walk_order* kernels: `ord`):
 *                      CS_WALK_CK  CS_WALK_UPTO  CS_WALK_RESTART  CS_WALK_STREAM
 *   cs_walk_clauses        0           0              0              0       csgpu_solve_many_clauses
 *   cs_walk_resume         1           0              0              0       one more argument, `ck`: the pool and the slots of the call
 *   cs_walk_upto           1           1              0              0       and `upto` (k >= 1, a scalar)
 *   cs_walk_restart        0           0              1              0       one more argument, `rs` (the walk is defined in csolve_gpu.h)
 *   cs_walk_stream         1           0              0              1       `ck` and `out`, the solution stream of the call
 *   cs_walk_order          0           0              0              0       one more argument, `ord`: the order, split_width, the halving counts
 *   cs_walk_order_resume   1           0              0              0       CS_WALK_ORDER 1 as well: `ck`, then `ord`
 *   cs_walk_order_from     1           0              0              0       CS_WALK_ORDER 1 and CS_WALK_FROM 1: `ck`, `ord`, `start`
 * Text, not a __device__ function, as cs_dive_body.hip.h.  Every line of a switch stands under its `#if`, so a kernel
 * that defines it 0 sees the text it saw before the switch was there and compiles to the same instructions.
 * CS_WALK_CK: an instance that stops at its budget leaves its frames, its current node, {bv, nv} and its incumbent in a
 * slot of the pool (the layout is in cs_walk.hip.h); with ck.resume the instances of ck.slots go on in their slots, which
 * are then their stacks.  New per-instance state is scalars only: slot, kept, depth0, nodes0, resumed, stack.
 * CS_WALK_UPTO: the ALL walk, left right after the k-th solution; solution j goes to row j of the instance's k rows, and
 * ck.capacity == 0 means "no pool" (pool, next and slots are not touched), so the one kernel serves the plain, the
 * checkpointed and the resume call.  It adds no per-instance state: the row index is inst, upto and sols, all scalar.
 * CS_WALK_RESTART: the ANY walk with a seeded rotation of every node's value order and Luby restarts, as CS_DIVE_RESTART
 * of cs_dive_body.hip.h.  nv is j, not a value, and a frame's 8-byte entry {variable, next j}; the call has n + 1 frames
 * per wave, the walk stays below frame n (io.frames - 1), and frame n keeps the root node's fixpoint, which a restart
 * reads back into the slice and into frame 0, every lane the entries it wrote itself.  A restart is no `continue` of the
 * ticket loop.  New per-instance state is scalars only: run, fails, threshold, counter, seed, restarts, start, width.
 * CS_WALK_STREAM: the ALL walk, every solution appended to `out` (io.all, io.solutions and ck.resume are not read).  Fresh
 * or resumed is a fact per instance, its ck.slots entry (-2 / >= 0).  A node without open variables asks for its row
 * BEFORE it is counted: without room a child goes round once more with `refused` set and leaves through the checkpoint
 * code of the budget, status 4, nv still that value; a root node leaves with zero fields and its slot entry -2.  New
 * per-instance state is scalars only: refused, room, the row index.
 * CS_WALK_FROM: the MIN / MAX walk of cs_walk_resume, one more argument `start` ([count] of cs_walk_start).  A fresh instance
 * with start[inst].have != 0 begins with that incumbent: have_best, best = start[inst].best, and dom[obj] of the root row
 * takes the objective bound before the root node's rounds, as a child's does (a bound that empties it fails in the first
 * round: DONE, no node).  io.best[inst] is written only when the instance has a solution of its own (sols > 0, the record's
 * count included when it is resumed): one that proves that nothing beats its start leaves best and its row alone.
 * ck.capacity == 0 means "no pool" as under CS_WALK_UPTO.  New per-instance state is scalars only: start_have, start_best.
 * CS_WALK_ORDER (a sixth switch; alone, every other switch 0, it is cs_walk_order): cs_walk_clauses's walk with one more
 * argument `ord` -- the branching variable is the open one with the smallest cs_order_key(ord.order, d) (cs_arith.h) in
 * place of the width in the two wave minima, and a node whose branching variable has more than ord.split_width values has
 * two children, [lo, mid] and [mid + 1, hi], mid = (lo + hi) >> 1 in 64 bits.  Kind and mid are read from the node as it
 * was entered (the slice when `fresh`, else its frame's row), before lane 0 writes the child and the incumbent's bound, so
 * a popped frame makes the same children; nv is the child's lower bound in both kinds, and a frame's entry {variable,
 * next}: the next value, or mid + 1.  io.frames is the host's bound (csgpu_many_clauses_ordered_frames).  New per-instance
 * state is scalars only: halvings, then.
 * CS_WALK_CK && CS_WALK_ORDER (cs_walk_order_resume alone): the ordered walk with cs_walk_resume's checkpoints.  A pushed
 * halving parent values no variable, so a slot has io.frames + 1 frames, not n + 1 (CS_WALK_SLOT), its depth is bounded
 * by io.frames, not n (CS_WALK_SLOT_FRAMES), and its header carries a magic of its own (CS_WALK_SLOT_MAGIC); the three
 * names stand for the old text in every other kernel.  ck.code is objective | order << 3, and a resumed instance's
 * halving count goes on from ord.halvings[inst].  A frame needs nothing new: {bv, nv} says where a halving node stands
 * (nv == lo: no half tried yet, nv == mid + 1: the second is next), kind and mid are read back from the frame's row.
 * CS_WALK_CK && CS_WALK_ORDER && CS_WALK_FROM (cs_walk_order_from alone): the two above together.  Every line of
 * CS_WALK_FROM stands under an `#if` of its own and reads nothing that CS_WALK_ORDER changes: the root row takes the start's
 * bound before the root node's rounds whatever the order, the header's incumbent is `best` / `have_best` (the start's until
 * the instance has a solution of its own), the report writes io.best at sols > 0 and ord.halvings beside it, and
 * ck.capacity == 0 draws no slot and leaves ck.slots alone.  A resumed instance reads ord.halvings[inst], so the host
 * requires the array with a pool; without one nothing is resumed and it may be NULL.
 * CS_WALK_WIDE (a seventh switch; cs_walk_wide with every other switch 0, cs_walk_wide_resume with CS_WALK_CK 1; the
 * nine kernels above define it 0):
 *                        CS_WALK_CK  CS_WALK_WIDE
 *   cs_walk_wide             0            1       cs_walk_clauses's arguments   csgpu_solve_many_clauses_wide
 *   cs_walk_wide_resume      1            1       cs_walk_resume's arguments    .._wide_checkpointed / _wide_resume
 * The clause records live in LDS, one copy per workgroup, not in a register array per lane, so the clause count has no
 * bound but the LDS of a CU.  The three register arrays and their load loop are gone; the workgroup stages
 * T.clause_by_kind (n_clauses records) and behind it T.lit (two literal records per CS_CL_OR2 clause) once, before its
 * waves draw their first ticket -- every thread its share, 16 bytes a load and a store -- and one __syncthreads() stands
 * between the copy and the ticket loop, which no wave can have left before.  Nothing writes the block afterwards.  The
 * waves' node slices lie behind it (a multiple of 16 bytes, so they stay 16-byte aligned), and the rounds are
 * cs_rounds_wide_body.hip.h.  No CPL: the kernels are templated on HAS_TREE alone.  The walk, the frames, the slots and
 * their magic, the counters and every store to device memory are the old text. */
  extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
  const int lane = threadIdx.x & (CS_WAVE - 1);
  const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wave_global = (int)blockIdx.x * CS_WAVES_PER_BLOCK + wave_in_block;
  const int n = T.n_vars;
  const size_t slice_al = ((size_t)n * sizeof(cs_val) + 16 + 15) & ~(size_t)15;
#if CS_WALK_WIDE
  /* the staged block: the clause records, then the literal records; the slices behind it */
  int4 *const wrec = (int4 *)cs_lds;
  int4 *const wlit = wrec + T.n_clauses;
  cs_val *dom = (cs_val *)(cs_lds + ((size_t)T.n_clauses + (size_t)T.n_lits) * sizeof(int4) + wave_in_block * slice_al);
#else
  cs_val *dom = (cs_val *)(cs_lds + wave_in_block * slice_al);
#endif
  unsigned *flag = (unsigned *)(dom + n); /* [0]: something changed this round */

#if CS_WALK_WIDE
  for (int i = (int)threadIdx.x; i < T.n_clauses; i += CS_BLOCK) wrec[i] = T.clause_by_kind[i];
  for (int i = (int)threadIdx.x; i < T.n_lits; i += CS_BLOCK) wlit[i] = T.lit[i];
  __syncthreads(); /* the one workgroup barrier: every wave is still here */
#else
  int4 rec[CPL], lit0[CPL], lit1[CPL];
#pragma unroll
  for (int q = 0; q < CPL; q++) {
    const int c = lane + q * CS_WAVE;
    rec[q] = c < T.n_clauses ? T.clause_by_kind[c] : make_int4(CS_CL_SKIP, 0, 0, 0);
    lit0[q] = rec[q].x == CS_CL_OR2 ? T.lit[rec[q].y] : make_int4(0, 0, 0, 0);
    lit1[q] = rec[q].x == CS_CL_OR2 ? T.lit[rec[q].y + 1] : make_int4(0, 0, 0, 0);
  }
#endif

  const int nsh = (int)gridDim.x < CS_DIVE_SHARDS ? (int)gridDim.x : CS_DIVE_SHARDS;
  const int shard = (int)(blockIdx.x % nsh);
  const unsigned count_x = io.count > shard ? (unsigned)((io.count - 1 - shard) / nsh + 1) : 0u; /* instances of this shard */
  const unsigned waves_x = (unsigned)((((int)gridDim.x - 1 - shard) / nsh + 1) * CS_WAVES_PER_BLOCK);
  unsigned *my_ticket = io.tickets + (size_t)shard * CS_DIVE_TICKET_STRIDE;
  const size_t fstride = (size_t)n + 1;
  cs_val *const wave_stack = io.stack + (size_t)wave_global * (size_t)io.frames * fstride;
  /* a slot's entries, the frames it has for a stack, and the word that marks its header */
#if CS_WALK_CK && CS_WALK_ORDER
#define CS_WALK_SLOT (((size_t)io.frames + 1) * fstride)
#define CS_WALK_SLOT_FRAMES io.frames
#define CS_WALK_SLOT_MAGIC CS_WALK_CK_MAGIC_ORDER
#else
#define CS_WALK_SLOT (fstride * fstride)
#define CS_WALK_SLOT_FRAMES n
#define CS_WALK_SLOT_MAGIC CS_WALK_CK_MAGIC
#endif

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

#if CS_WALK_RESTART
    unsigned run = 0u, rs_seed = rs.seed, start = 0u, width = 1u; /* scalars, as everything the restarts add */
    int restarts = 0;
    uint64_t fails = 0u, threshold = 1u, counter = 1u;
    if (rs.seeds != nullptr) rs_seed = (unsigned)__builtin_amdgcn_readfirstlane((int)rs.seeds[inst]);
    cs_val *const root_f = wave_stack + (size_t)(io.frames - 1) * fstride; /* the frame the walk leaves alone */
#endif
#if CS_WALK_CK
    /* the instance's slot (-1: none yet), the slot a checkpoint was written to in this launch, the stack the instance
     * walks on and, resuming, the checkpoint's depth and incumbent */
    int slot = -1, kept = -1, depth0 = 0, best0 = 0;
    bool resumed = false, have_best0 = false;
    cs_val *stack = wave_stack;
#if CS_WALK_STREAM
    /* the stream as it stands now (a relaxed load: a hint, the append itself decides), then what the instance is */
    const unsigned long long appended = (unsigned long long)cs_dive_uniform(
        (long long)__hip_atomic_load(out.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    slot = __builtin_amdgcn_readfirstlane(ck.slots[inst]);
    if (slot < 0 && slot != -2) continue; /* finished: nothing of it is read or written */
    if (appended >= (unsigned long long)out.capacity) { /* full already: no walk; an instance with a slot stays as it is */
      if (slot == -2 && lane == 0) {
        cs_dive_result res;
        res.status = 4; /* CSGPU_MANY_FULL */
        res.root_props = 0;
        res.nodes = 0; res.cuts = 0; res.props = 0; res.solutions = 0;
        io.results[inst] = res;
      }
      continue;
    }
    if (slot < 0) slot = -1; /* a fresh instance: it draws its slot when it stops */
    if (slot >= 0) {
#else
    if (ck.resume) {
      slot = __builtin_amdgcn_readfirstlane(ck.slots[inst]);
      if (slot < 0) continue; /* not stopped, or stopped without a checkpoint: nothing of it is written */
#endif
      cs_val head = cs_interval(-1, 0), inc = cs_interval(0, -2);
      if (slot < ck.capacity) { /* compared before it is read; the two header entries, nothing else of the slot yet */
        const cs_val *base = ck.pool + (size_t)slot * CS_WALK_SLOT;
        head = base[0];
        inc = base[1];
      }
      depth0 = __builtin_amdgcn_readfirstlane(head.lo);
      const int word = __builtin_amdgcn_readfirstlane(inc.hi); /* have_best | objective code << 1 */
      if (depth0 < 0 || depth0 >= CS_WALK_SLOT_FRAMES || __builtin_amdgcn_readfirstlane(head.hi) != CS_WALK_SLOT_MAGIC || (word >> 1) != ck.code) {
        if (lane == 0) io.results[inst].status = 3; /* CSGPU_MANY_BAD_SLOT */
        continue;
      }
      resumed = true;
      best0 = __builtin_amdgcn_readfirstlane(inc.lo);
      have_best0 = (word & 1) != 0;
      stack = ck.pool + (size_t)slot * CS_WALK_SLOT + fstride;
    }
#endif
#if CS_WALK_FROM
    /* the incumbent a fresh instance starts with: `have` as a scalar, and `best` only behind it */
    int start_have = 0, start_best = 0;
    if (!resumed) {
      start_have = __builtin_amdgcn_readfirstlane(start[inst].have);
      if (start_have != 0) start_best = __builtin_amdgcn_readfirstlane(start[inst].best);
    }
#endif
    /* the root row, into the LDS slice */
    bool bad_l = false;
#if CS_WALK_CK
    if (!resumed)
#endif
    for (int v = lane; v < n; v += CS_WAVE) {
      const cs_val d = io.roots[rrow + v], r = io.root_dom[v];
      bad_l = bad_l || d.lo > d.hi || d.lo < r.lo || d.hi > r.hi;
      dom[v] = d;
    }
    int status = 0 /* CSGPU_MANY_DONE */, root_props = 0;
    long long nodes = 0, cuts = 0, sols = 0, props = 0; /* scalars */
#if CS_WALK_ORDER
    long long halvings = 0; /* parents split in two */
#endif
    int acc_props = 0;                                  /* per lane, added to props every 64 nodes */
    int best = 0;
    bool have_best = false;
#if CS_WALK_FROM
    if (start_have != 0) { best = start_best; have_best = true; }
#endif
#if CS_WALK_CK
    long long nodes0 = 0; /* the nodes of earlier launches: the budget counts those of this one */
    if (resumed) {        /* the counters go on from the instance's record, the incumbent from the header */
      const cs_dive_result *was = io.results + inst;
      root_props = __builtin_amdgcn_readfirstlane(was->root_props);
      nodes0 = cs_dive_uniform(was->nodes);
      cuts = cs_dive_uniform(was->cuts);
      props = cs_dive_uniform(was->props);
      sols = cs_dive_uniform(was->solutions);
      nodes = nodes0;
#if CS_WALK_ORDER
      halvings = cs_dive_uniform(ord.halvings[inst]); /* the host requires the array: the count goes on as the record's do */
#endif
      best = best0;
      have_best = have_best0;
#if CS_WALK_UPTO
      have_best = false; /* an up-to-k walk has no incumbent, whatever the header says: obj_var is -1 */
#endif
#if CS_WALK_STREAM
      have_best = false; /* nor has the stream's ALL walk */
#endif
    }
#if CS_WALK_UPTO
    /* a resumed instance that holds its k solutions already (a smaller k than the slice before): DONE before it tries a
     * node, nothing of it is written but this.  It is what keeps the row index below k; unsigned, so that a negative
     * count in the caller's record ends here as well. */
    if (resumed && (unsigned long long)sols >= (unsigned long long)upto) {
      if (lane == 0) {
        io.results[inst].status = 0; /* CSGPU_MANY_DONE */
        ck.slots[inst] = -1;
      }
      continue;
    }
#endif
#endif

    if (__ballot(bad_l) != 0ull) {
      status = 2; /* CSGPU_MANY_BAD_ROOT */
    } else {
      /* One loop for the root node and every child, so that the rounds stand in the kernel once.  `root`: the node in
       * the slice is the root row itself, nothing is assigned and no node is counted.  f: the current node's frame. */
      int depth = 0, bv = 0, nv = 0;
      bool root = true, fresh = true; /* fresh: the slice holds the current node as it was entered */
      cs_val *f = wave_stack;
#if CS_WALK_ORDER
      int then = 0; /* what the current node tries after this child: the next value, or the second half's lower bound */
#endif
#if CS_WALK_STREAM
      bool refused = false; /* the child that was tried last is a solution the stream had no room for */
#endif
#if CS_WALK_CK
      if (resumed) { /* "try value nv of variable bv on the node in frame depth0", which is read into the slice */
        depth = depth0;
        f = stack + (size_t)depth0 * fstride;
        cs_val meta = cs_interval(0, 0);
        if (lane == 0) meta = f[n];
        bv = __builtin_amdgcn_readfirstlane(meta.lo);
        nv = __builtin_amdgcn_readfirstlane(meta.hi);
        /* cannot happen (the kernel wrote the slot): never index past the node.  As every bad slot, the status alone */
        if ((unsigned)bv >= (unsigned)n) {
          if (lane == 0) io.results[inst].status = 3; /* CSGPU_MANY_BAD_SLOT */
          continue;
        }
        root = false;
        fresh = false;
      }
#endif
#if CS_WALK_FROM
      /* the root row under the start incumbent: what a child gets, once every lane's part of the row stands in the slice */
      if (!resumed && have_best) {
        cs_wave_sync();
        if (lane == 0) dom[io.obj_var] = cs_objective_bound(io.sense, dom[io.obj_var], best);
      }
#endif
      for (;;) {
        depth = __builtin_amdgcn_readfirstlane(depth);
        bv = __builtin_amdgcn_readfirstlane(bv);
        nv = __builtin_amdgcn_readfirstlane(nv);
        bool last = false;
        if (!root) {
#if CS_WALK_CK
#if CS_WALK_STREAM
          if (refused || nodes - nodes0 >= io.max_nodes) {
            status = refused ? 4 /* CSGPU_MANY_FULL: nv is the refused value, the node in its frame is as it was */ : 1;
#else
          if (nodes - nodes0 >= io.max_nodes) {
            status = 1; /* CSGPU_MANY_LIMIT */
#endif
            /* leave a checkpoint, if the pool has a slot */
#if CS_WALK_UPTO
            if (ck.capacity > 0) /* no pool: no slot is drawn, the instance ends as without checkpoints */
#endif
#if CS_WALK_FROM
            if (ck.capacity > 0) /* the same */
#endif
            if (!resumed) {
              unsigned long long drawn = 0ull;
              if (lane == 0) drawn = __hip_atomic_fetch_add(ck.next, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              const unsigned dlo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)drawn);
              const unsigned dhi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(drawn >> 32));
              slot = dhi == 0u && dlo < (unsigned)ck.capacity ? (int)dlo : -1;
            }
            if (depth >= CS_WALK_SLOT_FRAMES) slot = -1; /* cannot happen (at most n frames in use; cs_walk_order_resume: io.frames): never write past the slot */
            if (slot >= 0) {
              cs_val *base = ck.pool + (size_t)slot * CS_WALK_SLOT;
              cs_val *frames = base + fstride;
              if (!resumed) { /* the frames in use and the current node's, every lane the entries it wrote */
                for (int d = 0; d <= depth; d++) {
                  const cs_val *src = wave_stack + (size_t)d * fstride;
                  cs_val *dst = frames + (size_t)d * fstride;
                  for (int v = lane; v < n; v += CS_WAVE) dst[v] = src[v];
                  if (lane == 0 && d < depth) dst[n] = src[n];
                }
              }
              if (lane == 0) {
                frames[(size_t)depth * fstride + n] = cs_interval(bv, nv);
                base[0] = cs_interval(depth, CS_WALK_SLOT_MAGIC);
                base[1] = cs_interval(best, (have_best ? 1 : 0) | (ck.code << 1));
              }
            }
            kept = slot;
            break;
          }
#else
          if (nodes >= io.max_nodes) { status = 1; /* CSGPU_MANY_LIMIT */ break; }
#endif
          if (!fresh) {
            for (int v = lane; v < n; v += CS_WAVE) dom[v] = f[v];
            cs_wave_sync();
          }
#if CS_WALK_RESTART
          /* where the value order of this node starts, from scalars: the node as it was entered is in the slice */
          const int xlo = __builtin_amdgcn_readfirstlane(dom[bv].lo), xhi = __builtin_amdgcn_readfirstlane(dom[bv].hi);
          width = (unsigned)xhi - (unsigned)xlo + 1u;
          start = (unsigned)cs_many_value(rs_seed, run, bv, cs_interval(xlo, xhi), 0u, rs.flags) - (unsigned)xlo;
          last = (unsigned)nv == width - 1u;
          const int value = cs_many_rotated(xlo, width, start, (unsigned)nv);
#elif CS_WALK_ORDER
          /* the node as it was entered says whether it halves, and where: scalars, 64-bit width and middle */
          const int xlo = __builtin_amdgcn_readfirstlane(dom[bv].lo), xhi = __builtin_amdgcn_readfirstlane(dom[bv].hi);
          const bool halves = (long long)xhi - (long long)xlo + 1 > (long long)ord.split_width;
          const int xmid = (int)(((long long)xlo + (long long)xhi) >> 1);
          const bool first_half = halves && nv == xlo;
          last = halves ? !first_half : nv == xhi;
          then = halves ? xmid + 1 : (int)((unsigned)nv + 1u); /* (not used after a last child: INT32_MAX wraps, unread) */
          const int child_hi = halves ? (first_half ? xmid : xhi) : nv;
          if (first_half) halvings++;
#else
          last = nv == __builtin_amdgcn_readfirstlane(dom[bv].hi);
#endif
          cs_wave_sync();
          if (lane == 0) {
#if CS_WALK_RESTART
            dom[bv] = cs_interval(value, value);
#elif CS_WALK_ORDER
            dom[bv] = cs_interval(nv, child_hi); /* the assignment, or the half: not counted in PROPS */
#else
            dom[bv] = cs_interval(nv, nv); /* the assignment: not counted in PROPS */
#endif
            if (have_best) dom[io.obj_var] = cs_objective_bound(io.sense, dom[io.obj_var], best);
          }
        }
        cs_wave_sync();

#if CS_WALK_WIDE
#include "cs_rounds_wide_body.hip.h"
#else
#include "cs_rounds_body.hip.h"
#endif
        (void)rounds;

        /* the open variables of a consistent node, and this lane's candidate for the branching variable */
        int open_vars = 0;
        unsigned kw = 0xffffffffu, kv = 0xffffffffu;
        if (!failed) {
          for (int v0 = 0; v0 < n; v0 += CS_WAVE) { /* uniform trips: the ballot counts every lane */
            const int v = v0 + lane;
            const cs_val d = v < n ? dom[v] : cs_value(0);
            const bool open = d.lo != d.hi;
#if CS_WALK_ORDER
            const unsigned w = cs_order_key(ord.order, d); /* below 0xffffffff for every open interval */
#else
            const unsigned w = (unsigned)d.hi - (unsigned)d.lo;
#endif
            if (open && w < kw) { kw = w; kv = (unsigned)v; }
            open_vars += __popcll(__ballot(open));
          }
        }
#if CS_WALK_STREAM
        /* a node that is a solution takes its row before any counter moves: one relaxed agent-scope add by lane 0, the
         * old value broadcast.  Refused, a child was not tried at all; a root node is not started (status FULL, the other
         * fields zero, its slot entry stays -2). */
        if (!failed && open_vars == 0) {
          __builtin_amdgcn_wave_barrier(); /* the wave meets before lane 0 adds, as in front of the ticket */
          unsigned long long at = 0ull;
          if (lane == 0) at =__hip_atomic_fetch_add(out.count, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          at = (unsigned long long)cs_dive_uniform((long long)at);
          const bool room = at < (unsigned long long)out.capacity;
          if (!room) {
            if (root) {
              status = 4; /* CSGPU_MANY_FULL */
              kept = -2;
              break;
            }
            refused = true;
            continue;
          }
          int *row = out.rows + (size_t)at * (size_t)n;
          for (int v = lane; v < n; v += CS_WAVE) row[v] = dom[v].lo;
          if (lane == 0) out.owner[at] = inst;
        }
#endif
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
#if CS_WALK_STREAM
          if (at_root) break; /* its row stands in the stream already; the root node was the one solution, else on (ALL) */
#elif CS_WALK_UPTO
          if (io.solutions != nullptr) { /* 1 <= sols <= upto here: a fresh count starts at 0, a resumed one below upto */
            const size_t srow = ((size_t)inst * (size_t)upto + (size_t)(sols - 1)) * (size_t)n;
            for (int v = lane; v < n; v += CS_WAVE) io.solutions[srow + v] = dom[v].lo;
          }
          if (sols >= (long long)upto || at_root) break; /* the k-th solution, or the root node was the one solution */
#else
          if (io.sense != 0) {
            best = __builtin_amdgcn_readfirstlane(dom[io.obj_var].lo);
            have_best = true;
          }
          if ((sols == 1 || io.sense != 0) && io.solutions != nullptr)
            for (int v = lane; v < n; v += CS_WAVE) io.solutions[rrow + v] = dom[v].lo;
          if (!io.all || at_root) break; /* ANY, or the root node was the one solution */
#endif
        }
#if CS_WALK_RESTART
        /* the root node's fixpoint, for the restarts */
        if (at_root && descend && rs.restart_base > 0)
          for (int v = lane; v < n; v += CS_WAVE) root_f[v] = dom[v];
        /* a failed child, unless it ends the whole tree: one more failure of this run, and past threshold x base the walk
         * starts again from the root node's fixpoint, with the next run's rotation.  No node, no rounds, no ticket: the
         * instance's own loop goes on. */
        bool again = false;
        if (!at_root && failed && !(last && depth == 0) && rs.restart_base > 0) {
          fails++;
          again = fails > threshold * (uint64_t)rs.restart_base;
        }
        if (again) {
          fails = 0u;
          cs_luby_next(&threshold, &counter);
          run++;
          restarts++;
          depth = 0;
          f = wave_stack;
          cs_wave_sync(); /* every lane has left the failed child */
          kw = 0xffffffffu; kv = 0xffffffffu;
          for (int v = lane; v < n; v += CS_WAVE) { /* the root has an open variable, or it would not have been kept */
            const cs_val d = root_f[v];
            dom[v] = d;
            f[v] = d;
            const unsigned w = (unsigned)d.hi - (unsigned)d.lo;
            if (d.lo != d.hi && w < kw) { kw = w; kv = (unsigned)v; }
          }
          cs_wave_sync();
          const unsigned wmin = cs_wave_min_u32(kw);
          bv = (int)cs_wave_min_u32(kw == wmin ? kv : 0xffffffffu);
          if ((unsigned)bv >= (unsigned)n) { status = 1; break; } /* cannot happen: never index past the node */
          nv = 0;
          fresh = true;
        } else
#endif
        if (descend) {
          if (!at_root && !last) { /* the parent comes back for its next value */
#if CS_WALK_ORDER
            if (lane == 0) f[n] = cs_interval(bv, then);
#else
            if (lane == 0) f[n] = cs_interval(bv, nv + 1);
#endif
            depth++;
            f += fstride;
          }
#if CS_WALK_RESTART
          if (depth >= io.frames - 1) { status = 1; break; } /* cannot happen (frames = n + 1); the last frame is the root node's */
#else
          if (depth >= io.frames) { status = 1; break; } /* cannot happen (frames = n; cs_walk_order: the host's bound): never write past the slice */
#endif
          for (int v = lane; v < n; v += CS_WAVE) f[v] = dom[v];
          const unsigned wmin = cs_wave_min_u32(kw);
          bv = (int)cs_wave_min_u32(kw == wmin ? kv : 0xffffffffu);
          /* cannot happen (an open variable exists): never index past the node */
          if ((unsigned)bv >= (unsigned)n) { status = 1; break; }
#if CS_WALK_RESTART
          nv = 0; /* j, not a value */
#else
          nv = __builtin_amdgcn_readfirstlane(dom[bv].lo);
#endif
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
#if CS_WALK_ORDER
          nv = then;
#else
          nv = nv + 1;
#endif
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
#if CS_WALK_FROM
      if (sols > 0 && io.best != nullptr) io.best[inst] = best; /* a solution of its own: never the start's value */
#else
      if (have_best && io.best != nullptr) io.best[inst] = best;
#endif
#if CS_WALK_RESTART
      if (rs.restarts != nullptr) rs.restarts[inst] = restarts;
#endif
#if CS_WALK_ORDER
      if (ord.halvings != nullptr) ord.halvings[inst] = halvings;
#endif
#if CS_WALK_UPTO
      if (ck.capacity > 0)
#endif
#if CS_WALK_FROM
      if (ck.capacity > 0)
#endif
#if CS_WALK_CK
      ck.slots[inst] = kept;
#endif
    }
    cs_wave_sync(); /* the next instance's root row goes into the slice only after every lane has left this one */
  }
#undef CS_WALK_SLOT_MAGIC
#undef CS_WALK_SLOT_FRAMES
#undef CS_WALK_SLOT
