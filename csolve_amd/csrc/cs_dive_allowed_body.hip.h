/* cs_dive_allowed_body.hip.h -- the body of the four kernels of cs_dive.hip.h that branch on the allowed values, which
 * includes it inside each of them under two switches:
 *                               CS_DIVE_CK  CS_DIVE_UPTO
 *   cs_dive_allowed                 0            0        csgpu_solve_many_allowed
 *   cs_dive_allowed_upto            0            1        csgpu_solve_many_allowed_upto: one more argument, `upto` (k >= 1, a scalar)
 *   cs_dive_allowed_resume          1            0        csgpu_solve_many_allowed_checkpointed / _resume: `ck`, the pool and the slots
 *   cs_dive_allowed_upto_resume     1            1        csgpu_solve_many_allowed_upto_checkpointed / _resume: `ck` and `upto`
 * Every line of CS_DIVE_CK stands under its `#if`: the two kernels that define it 0 see the text they saw before it.
 * CS_DIVE_CK: cs_dive_body.hip.h's checkpoints on this walk.  An instance that stops at max_nodes with work left draws a
 * slot and leaves there the header {depth, CS_DIVE_CK_MAGIC_ALLOWED}, its frames and the current node with {bv, nv}, nv the
 * lowest value still in aw (the budget is compared after the pop loop: aw is not empty there).  A resumed instance checks
 * slot number, magic and depth before anything else of the slot is read, walks in its slot, rebuilds the sets of the
 * current node and drops the bits below nv -- the pop path's own steps -- and goes on with the counters of its record.
 * A body of its own, not a fifth switch of cs_dive_body.hip.h: the five older kernels see the text they saw.  The ticket
 * loop, the root node, the child (assignment + cs_shave_core::fixpoint), the counters and the frames {row, bv, value + 1}
 * are those of cs_dive_body.hip.h with CS_DIVE_CK 0; text, not a function, for the reason given there.  What differs is
 * the branching (the walk is specified in csolve_gpu.h):
 *   entering a node, or coming back to a frame, every lane rebuilds the allowed values of its variables from the node's
 *   row (cs_dive_allowed_sets, cs_dive.hip.h); the branching variable is the wave minimum of (|allowed| - 1) << 8 | index;
 *   its allowed words go to NW scalars `aw`, the values still to be tried.  A child is the lowest bit of aw, which is then
 *   cleared; `last` is "aw is empty".  Coming back to a frame the bits below `next` are cleared.
 * New per-wave state across the child's fixpoint is scalars only (aw); the sets are dead once aw is read. */
  extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
  typedef unsigned long long u64;
  const int lane = threadIdx.x & (CS_WAVE - 1);
  const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves_per_block = blockDim.x >> 6;
  const int wave_global = (int)blockIdx.x * waves_per_block + wave_in_block;
  {
    const int vecs = (int)(tab_bytes / 16);
    const uint4 *src = (const uint4 *)tab_g;
    uint4 *dst = (uint4 *)cs_lds;
    for (int i = threadIdx.x; i < vecs; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();

  cs_shave_core<E, R, 0, false> C;
  C.s_tab = (const E *)cs_lds; C.slots = slots; C.lane = lane; C.s_trace = nullptr; C.tcount = 0u;
  int b0[R], h0[R];
  bool live[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int v = lane + r * CS_WAVE;
    live[r] = v < n;
    const int vc = live[r] ? v : n - 1;
    b0[r] = live[r] ? root_lo[vc] : 0;
    h0[r] = live[r] ? root_hi[vc] : 0;
    C.b0[r] = b0[r];
    C.kb[r] = b0[r] - dmin;
    C.deg[r] = live[r] ? sym_off[vc + 1] - sym_off[vc] : 0;
    C.livemask[r] = __ballot(live[r]);
  }

  const int nsh = (int)gridDim.x < CS_DIVE_SHARDS ? (int)gridDim.x : CS_DIVE_SHARDS;
  const int shard = (int)(blockIdx.x % nsh);
  const unsigned count_x = io.count > shard ? (unsigned)((io.count - 1 - shard) / nsh + 1) : 0u; /* instances of this shard */
  const unsigned waves_x = (unsigned)((((int)gridDim.x - 1 - shard) / nsh + 1) * waves_per_block);
  unsigned *my_ticket = io.tickets + (size_t)shard * CS_DIVE_TICKET_STRIDE;
  const size_t fstride = (size_t)n + 1;
#if CS_DIVE_CK
  cs_val *const wave_stack = io.stack + (size_t)wave_global * (size_t)io.frames * fstride;
#else
  cs_val *const stack = io.stack + (size_t)wave_global * (size_t)io.frames * fstride;
#endif

  /* the valued variables of the node in plo / phi and the allowed values of every open one (al) */
#define CS_DIVE_ASETS()                                                                                              \
  do {                                                                                                               \
    _Pragma("unroll") for (int r = 0; r < R; r++) pval[r] = __ballot(plo[r] == phi[r]) & C.livemask[r];              \
    cs_dive_allowed_sets<E, R, NW>(C, plo, phi, pval, al);                                                           \
  } while (0)
  /* the branching variable: the open variable with the fewest allowed values, ties to the lowest index */
#define CS_DIVE_ASELECT()                                                                                            \
  do {                                                                                                               \
    unsigned key_ = 0xffffffffu;                                                                                     \
    _Pragma("unroll") for (int r = R - 1; r >= 0; r--) {                                                             \
      const bool open_ = live[r] && plo[r] != phi[r];                                                                \
      int cnt_ = 0;                                                                                                  \
      _Pragma("unroll") for (int j = 0; j < NW; j++) cnt_ += __popc(al[r][j]);                                       \
      const unsigned k_ = ((unsigned)(cnt_ - 1) << 8) | (unsigned)(lane + r * CS_WAVE);                              \
      key_ = open_ && k_ < key_ ? k_ : key_;                                                                         \
    }                                                                                                                \
    bv = (int)(cs_wave_min_u32(key_) & 0xffu);                                                                       \
  } while (0)
  /* register, lane, bounds and allowed values of variable bv in the current node, as scalars */
#define CS_DIVE_AENTER()                                                                                             \
  do {                                                                                                               \
    br = bv >> 6;                                                                                                    \
    bl = bv & 63;                                                                                                    \
    _Pragma("unroll") for (int r = 0; r < R; r++) {                                                                  \
      if (r == br) {                                                                                                 \
        xlo = __builtin_amdgcn_readlane(plo[r], bl);                                                                 \
        bhi = __builtin_amdgcn_readlane(phi[r], bl);                                                                 \
        _Pragma("unroll") for (int j = 0; j < NW; j++)                                                               \
          aw[j] = (unsigned)__builtin_amdgcn_readlane((int)al[r][j], bl);                                            \
      }                                                                                                              \
    }                                                                                                                \
  } while (0)

  for (;;) {
    /* The wave meets here before lane 0 draws (cs_dive_body.hip.h: without this convergent no-op the loop gets a second
     * back edge for the other 63 lanes and the launch never ends). */
    __builtin_amdgcn_wave_barrier();
    unsigned t = 0u;
    if (lane == 0) t = __hip_atomic_fetch_add(my_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    if (t == count_x + waves_x - 1u && lane == 0) __hip_atomic_store(my_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t >= count_x) break;
    const int inst = (int)t * nsh + shard;
    const size_t rrow = (size_t)inst * (size_t)n;

    int plo[R], phi[R]; /* the current node, relative to the root lower bounds; a lane without a variable is the value 0 */
    bool bad_l = false;
#if CS_DIVE_CK
    /* the instance's slot (-1: none yet), the slot a checkpoint was written to in this launch, the stack the instance
     * walks on and, resuming, the checkpoint's depth */
    int slot = -1, kept = -1, depth0 = 0;
    cs_val *stack = wave_stack;
    bool resumed = false;
    if (ck.resume) {
      slot = __builtin_amdgcn_readfirstlane(ck.slots[inst]);
      if (slot < 0) continue; /* not stopped, or stopped without a checkpoint: nothing of it is written */
      cs_val head = cs_interval(-1, 0);
      if (slot < ck.capacity) head = ck.pool[(size_t)slot * (fstride * fstride)]; /* compared before it is read */
      depth0 = __builtin_amdgcn_readfirstlane(head.lo);
      if (depth0 < 0 || depth0 >= n || __builtin_amdgcn_readfirstlane(head.hi) != CS_DIVE_CK_MAGIC_ALLOWED) {
        if (lane == 0) io.results[inst].status = 3; /* CSGPU_MANY_BAD_SLOT */
        continue;
      }
      resumed = true;
      stack = ck.pool + (size_t)slot * (fstride * fstride) + fstride;
      const cs_val *f = stack + (size_t)depth0 * fstride; /* the current node */
#pragma unroll
      for (int r = 0; r < R; r++) {
        plo[r] = 0; phi[r] = 0;
        if (live[r]) {
          const cs_val d = f[lane + r * CS_WAVE];
          plo[r] = d.lo; phi[r] = d.hi;
        }
      }
    }
    if (!resumed)
#endif
    { /* a fresh instance: its root row */
#pragma unroll
      for (int r = 0; r < R; r++) {
        plo[r] = 0; phi[r] = 0;
        if (live[r]) {
          const cs_val d = io.roots[rrow + lane + r * CS_WAVE];
          bad_l = bad_l || d.lo > d.hi || d.lo < b0[r] || d.hi > h0[r];
          plo[r] = d.lo - b0[r];
          phi[r] = d.hi - b0[r];
        }
      }
    }
    int status = 0 /* CSGPU_MANY_DONE */, root_props = 0;
    long long nodes = 0, cuts = 0, sols = 0, props = 0; /* scalars */
    int acc_props = 0;                                  /* per lane, added to props every 64 nodes */
#if CS_DIVE_CK
    long long nodes0 = 0; /* the nodes of earlier launches: the budget counts those of this one */
    if (resumed) {        /* the counters go on from the instance's record */
      const cs_dive_result *was = io.results + inst;
      root_props = __builtin_amdgcn_readfirstlane(was->root_props);
      nodes0 = cs_dive_uniform(was->nodes);
      cuts = cs_dive_uniform(was->cuts);
      props = cs_dive_uniform(was->props);
      sols = cs_dive_uniform(was->solutions);
      nodes = nodes0;
    }
#if CS_DIVE_UPTO
    /* a resumed instance that holds its k solutions already (a smaller k than the slice before): DONE before it tries a
     * node, nothing of it is written but this; unsigned, so that a negative count in the caller's record ends here too */
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
#if CS_DIVE_CK
      int fail_var = -1;
      if (!resumed)
#else
      int fail_var;
#endif
      { /* the root node: nothing is taken for granted, every valued variable pushes */
        u64 pushed[R], push[R], dl[R], dh[R], val[R];
        int shaved = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
          pushed[r] = ~C.livemask[r];
          dl[r] = 0ull; dh[r] = 0ull;
          val[r] = __ballot(plo[r] == phi[r]) & C.livemask[r];
          push[r] = val[r];
          shaved -= phi[r] - plo[r];
        }
        int rounds = 0, revisions = 0;
        fail_var = C.fixpoint(plo, phi, pushed, push, dl, dh, val, rounds, revisions);
        if (rounds != 0) __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int r = 0; r < R; r++) shaved += phi[r] - plo[r];
        if (fail_var < 0) root_props = -cs_wave_sum(shaved);
      }
      int open_vars = 0;
#pragma unroll
      for (int r = 0; r < R; r++) open_vars += __popcll(__ballot(plo[r] != phi[r]));
      if (fail_var >= 0) {
        /* an inconsistent root: DONE, no node, no solution */
      } else if (open_vars == 0) {
        sols = 1;
        if (io.solutions != nullptr) {
#if CS_DIVE_UPTO
          const size_t row0 = (size_t)inst * (size_t)upto * (size_t)n; /* row 0 of the instance's k rows */
#else
          const size_t row0 = rrow;
#endif
#pragma unroll
          for (int r = 0; r < R; r++)
            if (live[r]) io.solutions[row0 + lane + r * CS_WAVE] = plo[r] + b0[r];
        }
      } else {
        int depth = 0, bv, br, bl, xlo = 0, bhi = 0;
        unsigned aw[NW]; /* the allowed values of bv that are still to be tried, bit k = root lower bound + k: scalars */
        unsigned al[R][NW];
        u64 pval[R];
#pragma unroll
        for (int j = 0; j < NW; j++) aw[j] = 0u;
#if CS_DIVE_CK
        if (resumed) { /* "go on at value nv of variable bv on the node plo / phi": the pop path's steps */
          depth = depth0;
          cs_val meta = cs_interval(0, 0);
          if (lane == 0) meta = stack[(size_t)depth0 * fstride + n];
          bv = __builtin_amdgcn_readfirstlane(meta.lo);
          const int nv = __builtin_amdgcn_readfirstlane(meta.hi);
          CS_DIVE_ASETS();
          CS_DIVE_AENTER();
          cs_dive_bits_from<NW>(aw, nv);
        } else
#endif
        {
          CS_DIVE_ASETS();
          CS_DIVE_ASELECT();
          CS_DIVE_AENTER();
        }
        for (;;) {
          depth = __builtin_amdgcn_readfirstlane(depth);
          bv = __builtin_amdgcn_readfirstlane(bv);
          /* Nothing left to try here (after a child that did not descend, or -- it cannot happen, a fixpoint's bounds are
           * allowed -- on a node or frame without an allowed value): back to the newest frame, at its first allowed value
           * >= next */
          bool finished = false;
          while (!cs_dive_any_bits<NW>(aw)) {
            if (depth == 0) { finished = true; break; }
            depth--;
            const cs_val *f = stack + (size_t)depth * fstride;
#pragma unroll
            for (int r = 0; r < R; r++) {
              plo[r] = 0; phi[r] = 0;
              if (live[r]) {
                const cs_val d = f[lane + r * CS_WAVE];
                plo[r] = d.lo; phi[r] = d.hi;
              }
            }
            cs_val meta = cs_interval(0, 0);
            if (lane == 0) meta = f[n];
            bv = __builtin_amdgcn_readfirstlane(meta.lo);
            const int next = __builtin_amdgcn_readfirstlane(meta.hi);
            CS_DIVE_ASETS();
            CS_DIVE_AENTER();
            cs_dive_bits_from<NW>(aw, next);
          }
          if (finished) break;
#if CS_DIVE_CK
          if (nodes - nodes0 >= io.max_nodes) {
            status = 1; /* CSGPU_MANY_LIMIT */
            { /* leave a checkpoint, if the pool has a slot */
              if (!resumed) {
                unsigned long long drawn = 0ull;
                if (lane == 0) drawn = __hip_atomic_fetch_add(ck.next, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned dlo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)drawn);
                const unsigned dhi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(drawn >> 32));
                slot = dhi == 0u && dlo < (unsigned)ck.capacity ? (int)dlo : -1;
              }
              if (depth >= n) slot = -1; /* cannot happen (at most n - 1 frames in use): never write past the slot */
              if (slot >= 0) {
                cs_val *base = ck.pool + (size_t)slot * (fstride * fstride);
                cs_val *frames = base + fstride;
                if (!resumed) { /* the frames in use, every lane the entries it wrote */
                  for (int d = 0; d < depth; d++) {
                    const cs_val *src = stack + (size_t)d * fstride;
                    cs_val *dst = frames + (size_t)d * fstride;
#pragma unroll
                    for (int r = 0; r < R; r++)
                      if (live[r]) dst[lane + r * CS_WAVE] = src[lane + r * CS_WAVE];
                    if (lane == 0) dst[n] = src[n];
                  }
                }
                unsigned rest[NW]; /* aw is not empty here: its lowest bit is the value the walk would try next */
#pragma unroll
                for (int j = 0; j < NW; j++) rest[j] = aw[j];
                const int nv = cs_dive_take_lowest<NW>(rest);
                cs_val *f = frames + (size_t)depth * fstride;
#pragma unroll
                for (int r = 0; r < R; r++)
                  if (live[r]) f[lane + r * CS_WAVE] = cs_interval(plo[r], phi[r]);
                if (lane == 0) {
                  f[n] = cs_interval(bv, nv);
                  base[0] = cs_interval(depth, CS_DIVE_CK_MAGIC_ALLOWED);
                }
              }
              kept = slot;
            }
            break;
          }
#else
          if (nodes >= io.max_nodes) {
            status = 1; /* CSGPU_MANY_LIMIT */
            break;
          }
#endif
          const int value = cs_dive_take_lowest<NW>(aw); /* relative to the root lower bound, as plo / phi are */
          const bool last = !cs_dive_any_bits<NW>(aw);
          int rlo[R], rhi[R];
          u64 pushed[R], push[R], dl[R], dh[R], val[R];
#pragma unroll
          for (int r = 0; r < R; r++) {
            rlo[r] = plo[r]; rhi[r] = phi[r];
            pushed[r] = pval[r] | ~C.livemask[r]; /* lanes without a variable look like values: they never push */
            push[r] = 0ull; dl[r] = 0ull; dh[r] = 0ull;
            val[r] = pval[r];
            if (r == br) {
              if (lane == bl) { rlo[r] = value; rhi[r] = value; }
              push[r] = 1ull << bl; /* a scalar shift */
              val[r] |= push[r];
            }
          }
          int rounds = 0, revisions = 0;
          const int fail_c = C.fixpoint(rlo, rhi, pushed, push, dl, dh, val, rounds, revisions);
          if (rounds != 0) __builtin_amdgcn_s_setprio(0);
          nodes++;
          bool descend = false;
          if (fail_c >= 0) {
            cuts++;
          } else {
            int open_c = 0;
#pragma unroll
            for (int r = 0; r < R; r++) {
              open_c += __popcll(__ballot(rlo[r] != rhi[r]));
              acc_props += (rlo[r] - plo[r]) + (phi[r] - rhi[r]); /* consistent children only: the reference's PROPS */
            }
            props -= bhi - xlo; /* the assignment itself is no narrowing */
            if (open_c == 0) {
              sols++;
#if CS_DIVE_UPTO
              if (io.solutions != nullptr) { /* 1 <= sols <= upto here */
                const size_t srow = ((size_t)inst * (size_t)upto + (size_t)(sols - 1)) * (size_t)n;
#pragma unroll
                for (int r = 0; r < R; r++)
                  if (live[r]) io.solutions[srow + lane + r * CS_WAVE] = rlo[r] + b0[r];
              }
              if (sols >= (long long)upto) break;
#else
              if (sols == 1 && io.solutions != nullptr) {
#pragma unroll
                for (int r = 0; r < R; r++)
                  if (live[r]) io.solutions[rrow + lane + r * CS_WAVE] = rlo[r] + b0[r];
              }
              if (!io.all) break;
#endif
            } else {
              descend = true;
            }
          }
          if ((nodes & 63) == 0) { props += cs_wave_sum(acc_props); acc_props = 0; }
          if (descend) {
            if (!last) { /* the node comes back for its next allowed value */
              if (depth >= io.frames) { status = 1; break; } /* cannot happen (frames >= n - 1): never write past the slice */
              cs_val *f = stack + (size_t)depth * fstride;
#pragma unroll
              for (int r = 0; r < R; r++)
                if (live[r]) f[lane + r * CS_WAVE] = cs_interval(plo[r], phi[r]);
              if (lane == 0) f[n] = cs_interval(bv, value + 1);
              depth++;
            }
#pragma unroll
            for (int r = 0; r < R; r++) { plo[r] = rlo[r]; phi[r] = rhi[r]; }
            CS_DIVE_ASETS();
            CS_DIVE_ASELECT();
            CS_DIVE_AENTER();
          }
        }
      }
    }
    props += cs_wave_sum(acc_props);
    if (lane == 0) {
      cs_dive_result res;
      res.status = status; res.root_props = root_props;
      res.nodes = nodes; res.cuts = cuts; res.props = props; res.solutions = sols;
      io.results[inst] = res;
#if CS_DIVE_CK
      ck.slots[inst] = kept;
#endif
    }
  }
#undef CS_DIVE_ASETS
#undef CS_DIVE_ASELECT
#undef CS_DIVE_AENTER
