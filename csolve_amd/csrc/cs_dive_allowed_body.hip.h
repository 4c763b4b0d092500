/* cs_dive_allowed_body.hip.h -- the body of the two kernels of cs_dive.hip.h that branch on the allowed values, which
 * includes it inside each of them under one switch:
 *                          CS_DIVE_UPTO
 *   cs_dive_allowed             0          csgpu_solve_many_allowed
 *   cs_dive_allowed_upto        1          csgpu_solve_many_allowed_upto: one more argument, `upto` (k >= 1, a scalar)
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
  cs_val *const stack = io.stack + (size_t)wave_global * (size_t)io.frames * fstride;

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
    int status = 0 /* CSGPU_MANY_DONE */, root_props = 0;
    long long nodes = 0, cuts = 0, sols = 0, props = 0; /* scalars */
    int acc_props = 0;                                  /* per lane, added to props every 64 nodes */

    if (__ballot(bad_l) != 0ull) {
      status = 2; /* CSGPU_MANY_BAD_ROOT */
    } else {
      int fail_var;
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
        CS_DIVE_ASETS();
        CS_DIVE_ASELECT();
        CS_DIVE_AENTER();
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
          if (nodes >= io.max_nodes) {
            status = 1; /* CSGPU_MANY_LIMIT */
            break;
          }
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
    }
  }
#undef CS_DIVE_ASETS
#undef CS_DIVE_ASELECT
#undef CS_DIVE_AENTER
