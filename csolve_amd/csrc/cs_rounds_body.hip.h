/* cs_rounds_body.hip.h -- the round loop of the clause-resident fixpoint, the one text of it.  Included inside
 * cs_propagate_clause_rounds (kernel 6, cs_kernels.hip.h) and inside cs_walk_clauses (cs_walk.hip.h), after the node
 * stands in the wave's LDS slice and a cs_wave_sync():
 *   reads    lane, n, dom, flag (LDS), rec[CPL], lit0[CPL], lit1[CPL], T, and the template parameters CPL, HAS_TREE
 *   leaves   cx (cx.props, cx.revisions: this lane's share of the node), rounds, failed (uniform), dom at the fixpoint
 *            (or with an emptied interval), and ends in a cs_wave_sync()
 * Text, not a __device__ function, as cs_dive_body.hip.h: kernel 6 sees the lines it always had and compiles to the
 * instructions it compiled to. */
    cs_ctx cx;
    cx.log = nullptr;
    cx.cur_clause = -1;
    cx.dom = dom;
    cx.mark = flag;
    cx.mark_is_flag = 1;
    cx.fail = 0;
    cx.fail_var = -1;
    cx.props = 0;
    cx.revisions = 0;
    int rounds = 0, failed = 0;
    for (;;) {
      if (lane == 0) flag[0] = 0u;
      /* an interval emptied by the assignment, the incumbent or racing updates of lo and hi */
      for (int v = lane; v < n; v += CS_WAVE)
        if (dom[v].lo > dom[v].hi) cx.failed_at(v);
      cs_wave_sync();
#pragma unroll
      for (int q = 0; q < CPL; q++) {
        /* a node that has failed in the slots so far is done (uniform); the relations sit in the first slots, `=` before
         * `<` before the disjunctions in the order the diverged lanes run, so the bounds a round's disjunctions see are
         * those the relations have just moved (schedule-12 MIN 1.49 -> 1.43 s; an exit between the relations and the
         * disjunctions of ONE slot costs more than it saves: 1.49 s) */
        if (q > 0 && __any(cx.fail)) break;
        if (cx.fail) break;
        const int4 r = rec[q];
        if (r.x == CS_CL_NE) {
          cs_ne_revise(cx, r.y, r.z, r.w);
        } else if (r.x == CS_CL_EQ || r.x == CS_CL_LT) {
          cs_lin_revise(cx, r.y, r.z, r.w, r.x == CS_CL_EQ ? CS_REL_EQ : CS_REL_LT);
        } else if (r.x == CS_CL_OR2) {
          const int4 lits[2] = { lit0[q], lit1[q] };
          cs_or2_revise(cx, lits);
        } else if (HAS_TREE && r.x == CS_CL_TREE) {
          cs_tree_scratch S; /* one lane interprets one expression tree: all trees of the model side by side */
          cs_tree_revise(T, r.y, cx, S);
        }
      }
      cs_wave_sync();
      if (__any(cx.fail)) { failed = 1; break; }
      if (flag[0] == 0u) break;
      rounds++;
    }
    cs_wave_sync();
