/* cs_rounds_wide_body.hip.h -- the round loop of cs_rounds_body.hip.h for clause records that live in LDS, one copy per
 * workgroup, in place of a register array per lane: no 512-clause limit.  Included inside cs_walk_body.hip.h under
 * CS_WALK_WIDE (cs_walk_wide, cs_walk_wide_resume), after the node stands in the wave's LDS slice and a cs_wave_sync():
 *   reads    lane, n, dom, flag (LDS), wrec[T.n_clauses], wlit[T.n_lits] (LDS, staged by the workgroup before its waves
 *            draw their first ticket and not written afterwards), T, and the template parameter HAS_TREE
 *   leaves   cx (cx.props, cx.revisions: this lane's share of the node), rounds, failed (uniform), dom at the fixpoint
 *            (or with an emptied interval), and ends in a cs_wave_sync()
 * Three things differ from cs_rounds_body.hip.h, everything else is its text: the slot loop runs q = 0 ..
 * ceil(n_clauses / 64) - 1 at run time (uniform: T is a kernel argument); the record of clause c = lane + 64 q is one
 * 16-byte LDS read -- lane-linear, so a wave's 1 KiB is conflict-free -- with CS_CL_SKIP past n_clauses; and the two
 * literal records of a CS_CL_OR2 clause are read from LDS as well, only by the lanes that hold one.  The order is
 * T.clause_by_kind's, so the lane-to-clause assignment and the order of the slots are kernel 6's, and so are the props. */
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
    const int wide_slots = (T.n_clauses + CS_WAVE - 1) / CS_WAVE;
    for (;;) {
      if (lane == 0) flag[0] = 0u;
      /* an interval emptied by the assignment, the incumbent or racing updates of lo and hi */
      for (int v = lane; v < n; v += CS_WAVE)
        if (dom[v].lo > dom[v].hi) cx.failed_at(v);
      cs_wave_sync();
      for (int q = 0; q < wide_slots; q++) {
        /* a node that has failed in the slots so far is done (uniform), as in cs_rounds_body.hip.h */
        if (q > 0 && __any(cx.fail)) break;
        if (cx.fail) break;
        const int c = lane + q * CS_WAVE;
        const int4 r = c < T.n_clauses ? wrec[c] : make_int4(CS_CL_SKIP, 0, 0, 0);
        if (r.x == CS_CL_NE) {
          cs_ne_revise(cx, r.y, r.z, r.w);
        } else if (r.x == CS_CL_EQ || r.x == CS_CL_LT) {
          cs_lin_revise(cx, r.y, r.z, r.w, r.x == CS_CL_EQ ? CS_REL_EQ : CS_REL_LT);
        } else if (r.x == CS_CL_OR2) {
          const int4 lits[2] = { wlit[r.y], wlit[r.y + 1] };
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
