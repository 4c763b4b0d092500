/* cs_dive_body.hip.h -- the body of the five kernels of cs_dive.hip.h, which includes it inside each of them under four
 * switches:            CS_DIVE_CK  CS_DIVE_UPTO  CS_DIVE_RESTART  CS_DIVE_STREAM
 *   cs_dive_shave          0           0              0              0       csgpu_solve_many
 *   cs_dive_resume         1           0              0              0       one more argument, `ck`: the pool and the slots of the call
 *   cs_dive_upto           1           1              0              0       and `upto` (k >= 1, a scalar)
 *   cs_dive_restart        0           0              1              0       one more argument, `rs` (the walk is defined in csolve_gpu.h)
 *   cs_dive_stream         1           0              0              1       `ck` and `out`, the solution stream of the call
 * Text, not a __device__ function: inlined from a function, the loop of cs_dive_shave<E, 2> takes 42 vector registers
 * instead of 39.  Every line of a switch stands under its `#if`, so a kernel that defines it 0 sees the text it saw before
 * the switch was there and compiles to the same instructions.
 * CS_DIVE_UPTO: the instance stops right after its k-th solution, solution j goes to row j of the instance's k rows, and
 * io.all is not read.  A pool of capacity 0 means "no pool": ck.next, ck.pool and ck.slots are then never touched.
 * CS_DIVE_RESTART: the ANY walk with a seeded rotation of every node's value order and Luby restarts.  A frame's 8-byte
 * entry is {variable, next j} instead of {variable, next value}; the root node's fixpoint is kept in frame `frames - 1`,
 * which the walk never uses, and a restart reads it back, every lane the entries it wrote itself.  A restart is no
 * `continue` of the ticket loop.  New per-wave state is scalars only: run, fails, threshold, counter, seed, restarts, start.
 * CS_DIVE_STREAM: the ALL walk, every solution appended to `out` (io.all, io.solutions and ck.resume are not read).  Fresh
 * or resumed is a fact per instance, its ck.slots entry (-2 / >= 0).  A child that is a solution asks for its row BEFORE it
 * is counted: without room the walk goes round once more with `refused` set and leaves through the checkpoint code of the
 * budget, status 4, nv still that value.  New per-wave state is scalars only: refused, room, the row index. */
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
  cs_val *const wave_stack = io.stack + (size_t)wave_global * (size_t)io.frames * fstride;

  /* the branching variable of the node in plo / phi (an open variable exists) and the valued variables of the node (a
   * macro: a lambda that changes captured scalars leaves them in scratch memory) */
#define CS_DIVE_SELECT()                                                                                             \
  do {                                                                                                               \
    unsigned key_ = 0xffffffffu;                                                                                     \
    _Pragma("unroll") for (int r = R - 1; r >= 0; r--) {                                                             \
      const bool open_ = live[r] && plo[r] != phi[r];                                                                \
      const unsigned k_ = ((unsigned)(phi[r] - plo[r]) << 8) | (unsigned)(lane + r * CS_WAVE);                       \
      key_ = open_ && k_ < key_ ? k_ : key_;                                                                         \
    }                                                                                                                \
    bv = (int)(cs_wave_min_u32(key_) & 0xffu);                                                                       \
  } while (0)
  /* register, lane and bounds of variable bv in the current node; the node's valued variables */
#define CS_DIVE_ENTER()                                                                                              \
  do {                                                                                                               \
    br = bv >> 6;                                                                                                    \
    bl = bv & 63;                                                                                                    \
    _Pragma("unroll") for (int r = 0; r < R; r++) {                                                                  \
      pval[r] = __ballot(plo[r] == phi[r]) & C.livemask[r];                                                          \
      if (r == br) {                                                                                                 \
        xlo = __builtin_amdgcn_readlane(plo[r], bl);                                                                 \
        bhi = __builtin_amdgcn_readlane(phi[r], bl);                                                                 \
      }                                                                                                              \
    }                                                                                                                \
  } while (0)
#if CS_DIVE_RESTART
  /* where the value order of the entered node starts: from scalars, once per node (cs_arith.h) */
#define CS_DIVE_START()                                                                                              \
  do {                                                                                                               \
    width = (unsigned)(bhi - xlo) + 1u;                                                                              \
    start = cs_many_start(rs_seed, run, bv, width, rs.flags);                                                        \
  } while (0)
#endif
#if CS_DIVE_STREAM
  /* the solution LO (relative to the root lower bounds) asks for a row of the stream: one relaxed agent-scope add by
   * lane 0, the old value broadcast; ROOM = it lies below the capacity, and then the row and its owner are stored */
#define CS_DIVE_APPEND(LO, ROOM)                                                                                     \
  do {                                                                                                               \
    u64 at_ = 0ull;                                                                                                  \
    if (lane == 0) at_ = __hip_atomic_fetch_add(out.count, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        \
    at_ = (u64)cs_dive_uniform((long long)at_);                                                                      \
    ROOM = at_ < (u64)out.capacity;                                                                                  \
    if (ROOM) {                                                                                                      \
      int *row_ = out.rows + (size_t)at_ * (size_t)n;                                                                \
      _Pragma("unroll") for (int r = 0; r < R; r++)                                                                  \
        if (live[r]) row_[lane + r * CS_WAVE] = LO[r] + b0[r];                                                       \
      if (lane == 0) out.owner[at_] = inst;                                                                          \
    }                                                                                                                \
  } while (0)
#endif

  for (;;) {
    /* The wave meets here before lane 0 draws.  Without this convergent no-op the compiler joins the `lane == 0` of
     * the result store at the end of the body with the `lane == 0` of the draw, gives the loop a second back edge for
     * the other 63 lanes and lets them go round alone with ticket 0: the launch never ends (seen in the ISA). */
    __builtin_amdgcn_wave_barrier();
    unsigned t = 0u;
    if (lane == 0) t = __hip_atomic_fetch_add(my_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    if (t == count_x + waves_x - 1u && lane == 0) __hip_atomic_store(my_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t >= count_x) break;
    const int inst = (int)t * nsh + shard;
    const size_t rrow = (size_t)inst * (size_t)n;

#if CS_DIVE_RESTART
    unsigned run = 0u, rs_seed = rs.seed, start = 0u, width = 1u; /* scalars, as everything the restarts add */
    int restarts = 0;
    uint64_t fails = 0u, threshold = 1u, counter = 1u;
    if (rs.seeds != nullptr) rs_seed = (unsigned)__builtin_amdgcn_readfirstlane((int)rs.seeds[inst]);
#endif
    int plo[R], phi[R]; /* the current node, relative to the root lower bounds; a lane without a variable is the value 0 */
    bool bad_l = false;
#if CS_DIVE_CK
    /* the instance's slot (-1: none yet), the slot a checkpoint was written to in this launch, the stack the instance
     * walks on and, resuming, the checkpoint's depth */
    int slot = -1, kept = -1, depth0 = 0;
    cs_val *stack = wave_stack;
    bool resumed = false;
    {
#if CS_DIVE_STREAM
      /* the stream as it stands now (a relaxed load: a hint, the append itself decides), then what the instance is */
      const u64 appended = (u64)cs_dive_uniform((long long)__hip_atomic_load(out.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      slot = __builtin_amdgcn_readfirstlane(ck.slots[inst]);
      if (slot < 0 && slot != -2) continue; /* finished: nothing of it is read or written */
      if (appended >= (u64)out.capacity) { /* full already: no walk; an instance with a slot stays exactly as it is */
        if (slot == -2 && lane == 0) {
          cs_dive_result res;
          res.status = 4; /* CSGPU_MANY_FULL */
          res.root_props = 0;
          res.nodes = 0; res.cuts = 0; res.props = 0; res.solutions = 0;
          io.results[inst] = res;
        }
        continue;
      }
      if (slot >= 0) {
#else
      if (ck.resume) {
        slot = __builtin_amdgcn_readfirstlane(ck.slots[inst]);
        if (slot < 0) continue; /* not stopped, or stopped without a checkpoint: nothing of it is written */
#endif
        cs_val head = cs_interval(-1, 0);
        if (slot < ck.capacity) head = ck.pool[(size_t)slot * (fstride * fstride)]; /* compared before it is read */
        depth0 = __builtin_amdgcn_readfirstlane(head.lo);
        if (depth0 < 0 || depth0 >= n || __builtin_amdgcn_readfirstlane(head.hi) != CS_DIVE_CK_MAGIC) {
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
#if CS_DIVE_STREAM
      else {
        slot = -1; /* a fresh instance: it draws its slot when it stops */
      }
#endif
    }
#else
    cs_val *const stack = wave_stack;
    const bool resumed = false;
    const int depth0 = 0;
#endif
    if (!resumed) {
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
    {
      if (resumed) { /* the counters go on from the instance's record */
        const cs_dive_result *was = io.results + inst;
        root_props = __builtin_amdgcn_readfirstlane(was->root_props);
        nodes0 = cs_dive_uniform(was->nodes);
        cuts = cs_dive_uniform(was->cuts);
        props = cs_dive_uniform(was->props);
        sols = cs_dive_uniform(was->solutions);
        nodes = nodes0;
      }
    }
#if CS_DIVE_UPTO
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
#else
    const long long nodes0 = 0;
#endif

    if (__ballot(bad_l) != 0ull) {
      status = 2; /* CSGPU_MANY_BAD_ROOT */
    } else {
#if CS_DIVE_CK
      int fail_var = -1;
      if (!resumed)
#else
      int fail_var; /* (left without a value as it always was: with one, cs_dive_shave's scalar registers are allotted anew) */
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
      int open_vars = 0; /* (a checkpoint's current node has one: the variable it branches on) */
#pragma unroll
      for (int r = 0; r < R; r++) open_vars += __popcll(__ballot(plo[r] != phi[r]));
      if (fail_var >= 0) {
        /* an inconsistent root: DONE, no node, no solution */
      } else if (open_vars == 0) {
#if CS_DIVE_STREAM
        /* the root row is itself the solution (a fresh instance: a checkpoint's node has an open variable).  Without
         * room it is not started: status FULL, the other fields zero, its slot entry stays -2 */
        bool room;
        CS_DIVE_APPEND(plo, room);
        if (room) {
          sols = 1;
        } else {
          status = 4; /* CSGPU_MANY_FULL */
          root_props = 0;
          kept = -2;
        }
#else
        sols = 1;
        if (io.solutions != nullptr) {
#if CS_DIVE_UPTO
          const size_t row0 = (size_t)inst * (size_t)upto * (size_t)n; /* row 0 of the instance's k rows */
#pragma unroll
          for (int r = 0; r < R; r++)
            if (live[r]) io.solutions[row0 + lane + r * CS_WAVE] = plo[r] + b0[r];
#else
#pragma unroll
          for (int r = 0; r < R; r++)
            if (live[r]) io.solutions[rrow + lane + r * CS_WAVE] = plo[r] + b0[r];
#endif
        }
#endif
      } else {
        int depth = 0, bv, br, bl, xlo = 0, bhi = 0, nv;
#if CS_DIVE_STREAM
        bool refused = false; /* the child that was tried last is a solution the stream had no room for */
#endif
        u64 pval[R];
        if (resumed) { /* "try value nv of variable bv on the node plo / phi" */
          depth = depth0;
          cs_val meta = cs_interval(0, 0);
          if (lane == 0) meta = stack[(size_t)depth0 * fstride + n];
          bv = __builtin_amdgcn_readfirstlane(meta.lo);
          nv = __builtin_amdgcn_readfirstlane(meta.hi);
          CS_DIVE_ENTER();
        } else {
          CS_DIVE_SELECT();
          CS_DIVE_ENTER();
#if CS_DIVE_RESTART
          CS_DIVE_START();
          nv = 0; /* j, not a value */
#else
          nv = xlo;
#endif
        }
#if CS_DIVE_RESTART
        /* the root node's fixpoint, for the restarts: the frame the walk leaves alone */
        cs_val *const root_f = stack + (size_t)(io.frames - 1) * fstride;
        if (rs.restart_base > 0) {
#pragma unroll
          for (int r = 0; r < R; r++)
            if (live[r]) root_f[lane + r * CS_WAVE] = cs_interval(plo[r], phi[r]);
        }
#endif
        for (;;) {
          depth = __builtin_amdgcn_readfirstlane(depth);
          nv = __builtin_amdgcn_readfirstlane(nv);
          bv = __builtin_amdgcn_readfirstlane(bv);
#if CS_DIVE_STREAM
          if (refused || nodes - nodes0 >= io.max_nodes) {
            status = refused ? 4 /* CSGPU_MANY_FULL: nv is the refused value, the node is as it was */ : 1;
#else
          if (nodes - nodes0 >= io.max_nodes) {
            status = 1; /* CSGPU_MANY_LIMIT */
#endif
#if CS_DIVE_CK
            { /* leave a checkpoint, if the pool has a slot */
#if CS_DIVE_UPTO
              if (ck.capacity > 0) /* no pool: no slot is drawn, the instance ends as without checkpoints */
#endif
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
                cs_val *f = frames + (size_t)depth * fstride;
#pragma unroll
                for (int r = 0; r < R; r++)
                  if (live[r]) f[lane + r * CS_WAVE] = cs_interval(plo[r], phi[r]);
                if (lane == 0) {
                  f[n] = cs_interval(bv, nv);
                  base[0] = cs_interval(depth, CS_DIVE_CK_MAGIC);
                }
              }
              kept = slot;
            }
#endif
            break;
          }
#if CS_DIVE_RESTART
          const int value = cs_many_rotated(xlo, width, start, (unsigned)nv);
          const bool last = (unsigned)nv == width - 1u;
#else
          const int value = nv;
          const bool last = value == bhi;
#endif
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
          const int fail_var = C.fixpoint(rlo, rhi, pushed, push, dl, dh, val, rounds, revisions);
          if (rounds != 0) __builtin_amdgcn_s_setprio(0);
#if CS_DIVE_STREAM
          /* a child that is a solution takes its row before any counter moves: refused, it was not tried at all */
          if (fail_var < 0) {
            int open_s = 0;
#pragma unroll
            for (int r = 0; r < R; r++) open_s += __popcll(__ballot(rlo[r] != rhi[r]));
            if (open_s == 0) {
              bool room;
              CS_DIVE_APPEND(rlo, room);
              if (!room) {
                refused = true;
                continue;
              }
            }
          }
#endif
          nodes++;
          bool descend = false;
          if (fail_var >= 0) {
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
#if CS_DIVE_STREAM
              /* its row stands in the stream already; the walk goes on (ALL) */
#elif CS_DIVE_UPTO
              if (io.solutions != nullptr) { /* 1 <= sols <= upto here: a fresh count starts at 0, a resumed one below upto */
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
#if CS_DIVE_RESTART
          /* a failed child (ANY: whatever does not descend here has failed), unless it ends the whole tree: one more
           * failure of this run, and past threshold x base the walk starts again from the root node's fixpoint, with
           * the next run's rotation.  No node, no ticket: the instance's own loop goes on. */
          bool again = false;
          if (!descend && !(last && depth == 0) && rs.restart_base > 0) {
            fails++;
            again = fails > threshold * (uint64_t)rs.restart_base;
          }
          if (again) {
            fails = 0u;
            cs_luby_next(&threshold, &counter);
            run++;
            restarts++;
            depth = 0;
#pragma unroll
            for (int r = 0; r < R; r++) {
              plo[r] = 0; phi[r] = 0;
              if (live[r]) {
                const cs_val d = root_f[lane + r * CS_WAVE];
                plo[r] = d.lo; phi[r] = d.hi;
              }
            }
            CS_DIVE_SELECT();
            CS_DIVE_ENTER();
            CS_DIVE_START();
            nv = 0;
          } else
#endif
          if (descend) {
            if (!last) { /* the node comes back for its next value */
#if CS_DIVE_RESTART
              if (depth >= io.frames - 1) { status = 1; break; } /* cannot happen; the last frame is the root node's */
#else
              if (depth >= io.frames) { status = 1; break; } /* cannot happen (frames >= n - 1): never write past the slice */
#endif
              cs_val *f = stack + (size_t)depth * fstride;
#pragma unroll
              for (int r = 0; r < R; r++)
                if (live[r]) f[lane + r * CS_WAVE] = cs_interval(plo[r], phi[r]);
#if CS_DIVE_RESTART
              if (lane == 0) f[n] = cs_interval(bv, nv + 1);
#else
              if (lane == 0) f[n] = cs_interval(bv, value + 1);
#endif
              depth++;
            }
#pragma unroll
            for (int r = 0; r < R; r++) { plo[r] = rlo[r]; phi[r] = rhi[r]; }
            CS_DIVE_SELECT();
            CS_DIVE_ENTER();
#if CS_DIVE_RESTART
            CS_DIVE_START();
            nv = 0;
#else
            nv = xlo;
#endif
          } else if (last) { /* the node's values are used up */
            if (depth == 0) break;
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
            nv = __builtin_amdgcn_readfirstlane(meta.hi);
            CS_DIVE_ENTER();
#if CS_DIVE_RESTART
            CS_DIVE_START(); /* the run is the one that pushed the frame: a restart empties the stack */
#endif
          } else {
#if CS_DIVE_RESTART
            nv = nv + 1;
#else
            nv = value + 1;
#endif
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
#if CS_DIVE_RESTART
      if (rs.restarts != nullptr) rs.restarts[inst] = restarts;
#endif
#if CS_DIVE_UPTO
      if (ck.capacity > 0)
#endif
#if CS_DIVE_CK
      ck.slots[inst] = kept;
#endif
    }
  }
#undef CS_DIVE_SELECT
#undef CS_DIVE_ENTER
#if CS_DIVE_RESTART
#undef CS_DIVE_START
#endif
#if CS_DIVE_STREAM
#undef CS_DIVE_APPEND
#endif
