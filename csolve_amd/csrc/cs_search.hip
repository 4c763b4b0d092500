/* cs_search.hip -- device-resident tree search on top of the batched propagation ABI.
 * Reference behaviour being mirrored: solve() (reference src/csolve.c:398-476) -- branch on a
 * variable, try every value of its interval (step_val 331-338), propagate each (check_assignment
 * 247-261), count CALLS/CUTS (65-73, 255-258), accept complete assignments whose root evaluates to
 * true (update_solution 222-244), keep the incumbent (objective.c:81-126).  The reference walks
 * this tree depth-first one node at a time; here whole frontiers are expanded per launch. */
#include <hip/hip_runtime.h>
#include <chrono>
#include <type_traits>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/csolve_gpu.h"
#include "cs_arith.h"
#include "cs_frontend.h"
#include "cs_internal.h"

#include "cs_search_kernels.hip.h"

/* the environment switches of an engine, read once by csgpu_search_create: callers, the tests among
 * them, set them before they create an engine */
struct cs_search_switches {
  int burst_off;       /* CSGPU_SEARCH_BURST=0: every iteration driven from the host */
  int graph_off;       /* CSGPU_SEARCH_GRAPH=0: the launches of a burst enqueued one by one */
  int burst_split;     /* MIN / MAX: a device-driven iteration's bookkeeping by several workgroups (BURST_SPLIT=0: one) */
  int eval_always;     /* CSGPU_SEARCH_EVAL=1: complete children of pure != networks are evaluated all the same (tests) */
  int holes_off;       /* CSGPU_SEARCH_HOLES=0: a child for every value of the interval, none cut by the parent's set */
  int sets_off;        /* CSGPU_SEARCH_SETS=0: interval rows only in the pool of the separate-kernel path too */
  int fused_off;       /* CSGPU_SEARCH_FUSED=0: ALL through the separate kernels, not the level kernels */
  int trace;           /* CSGPU_SEARCH_TRACE set: device-side state after every burst / frontier to stderr */
  int64_t parents_max; /* tuning (PARENTS_MAX): parents of a device-driven MIN / MAX iteration, see search_init */
  int64_t backlog_div; /* tuning (BACKLOG_DIV): B_BACKLOG_DIV of a burst, a quarter of the pool (was a sixteenth) */
  int64_t stage_mult;  /* tuning (CSGPU_STEP_STAGE_MULT): staging rows of the level kernels per max_children */
};

static int env_is(const char *name, char c) {
  const char *e = getenv(name);
  return e != NULL && e[0] == c;
}
static int64_t env_count(const char *name, int64_t otherwise) { /* a count of at least 1, or `otherwise` */
  const char *e = getenv(name);
  return e != NULL && atoll(e) >= 1 ? atoll(e) : otherwise;
}

static cs_search_switches read_switches(void) {
  cs_search_switches w;
  w.burst_off = env_is("CSGPU_SEARCH_BURST", '0');
  w.graph_off = env_is("CSGPU_SEARCH_GRAPH", '0');
  w.burst_split = !env_is("CSGPU_SEARCH_BURST_SPLIT", '0');
  w.eval_always = env_is("CSGPU_SEARCH_EVAL", '1');
  w.holes_off = env_is("CSGPU_SEARCH_HOLES", '0');
  w.sets_off = env_is("CSGPU_SEARCH_SETS", '0');
  w.fused_off = env_is("CSGPU_SEARCH_FUSED", '0');
  w.trace = getenv("CSGPU_SEARCH_TRACE") != NULL;
  w.parents_max = env_count("CSGPU_SEARCH_PARENTS_MAX", 8192);
  w.backlog_div = env_count("CSGPU_SEARCH_BACKLOG_DIV", 4);
  w.stage_mult = env_count("CSGPU_STEP_STAGE_MULT", 2);
  return w;
}

/* how an engine iterates, decided by plan_path alone */
enum cs_path {
  PATH_LEVELS,      /* ALL on a model with a step kernel: one level kernel per frontier (one_iteration_fused) */
  PATH_HOST,        /* host-driven iterations (one_iteration), small or large by their parent count */
  PATH_BURST_ONE,   /* device-driven bursts, bookkeeping by one workgroup (cs_expand_burst, cs_classify_small) */
  PATH_BURST_SPLIT, /* device-driven MIN / MAX bursts, bookkeeping over several workgroups (cs_burst_*) */
};

struct csgpu_search {
  const csgpu_model *m;
  int n, objective, obj_var;
  int64_t cap, max_children, max_parents, max_width, parents_limit;
  int64_t parents_max; /* device-driven iterations take up to this many parents when the pool has a backlog */
  double avg_children; /* children per parent of the recent iterations (ALL sizes its batches by it) */
  cs_val *pool;
  int64_t top, peak;
  /* forbidden sets travelling with the states (pure binary-NE models, csgpu_propagate_batch_fb) */
  int fw;
  unsigned long long *pool_forb, *d_child_forb;
  csgpu_node *d_rebuild_nodes;
  cs_choice *d_choice; /* per parent: what cs_branch decided */
  int *d_child_off /* per workgroup of cs_branch */, *d_block_sum, *d_block_skip;
  csgpu_node *d_nodes;
  cs_val *d_child_states, *d_complete_states;
  csgpu_result *d_results;
  int *d_dest /* survivor k = child d_dest[k] */, *d_complete_list, *d_truth;
  int *d_block_surv, *d_block_comp, *d_block_cuts, *d_block_props, *d_block_revs, *d_surv_off, *d_comp_off;
  unsigned long long *d_counters; /* [C_COUNT] */
  int *d_best;                    /* = (int *)&d_counters[C_BEST] */
  int64_t pending_complete;       /* complete children of the last iteration whose accept results are unread */
  int32_t *d_solutions;           /* [max_solutions][n] */
  int32_t *d_best_solution;       /* [n] a solution attaining the incumbent (MIN/MAX) */
  int have_best_solution;
  int32_t best_solution_value;    /* the objective value d_best_solution attains (it may have been overtaken by an engine
                                   * that shares the incumbent word: then this engine has no best row to show) */
  /* a shared incumbent (csgpu_search_share_incumbent): the engine whose word this one uses, and how many engines
   * use this one's.  A lender is kept alive (csgpu_search_free deferred) until its last borrower is gone. */
  csgpu_search *lender;
  int borrowers, free_pending;
  double put_seconds;     /* host time spent in csgpu_search_put / put_host (copy + rebuilding the forbidden sets) */
  int64_t put_states;
  int device; /* the device the engine was created on; made current in the calling thread by every entry point
               * (a fresh host thread starts on device 0) */
  int64_t max_solutions;
  csgpu_search_stats st;
  /* restarts (ANY): the states put from outside are kept to restart from */
  cs_val *seed;
  int64_t seed_count, seed_cap, restart_base, since_restart;
  uint64_t luby_threshold, luby_counter;
  /* device-driven iterations (ANY / MIN / MAX): BURST_ITERATIONS iterations per host round trip, as one hipGraph */
  unsigned long long *d_burst, *h_burst; /* [B_COUNT] device / pinned host; h_burst[B_COUNT ...] = copy of the counters,
                                          * then the incumbent */
  hipStream_t burst_stream;
  hipGraphExec_t burst_exec;
  int64_t burst_limit; /* parents per iteration the graph was built for (0: none) */
  cs_holes holes;      /* values a parent's own set forbids are cut without a launch (one set word per variable) */
  /* fused levels (cs_step.hip.h): ALL on models with a step kernel -- the pool holds interval rows only, a frontier is
   * one launch (branch + fixpoints + store) plus cs_collect */
  int counted; /* this engine is in its model's engine count */
  int64_t stage_rows;           /* rows of d_child_states, the staging buffer of the survivors */
  uint32_t *d_fill, *d_ticket;
  uint64_t *d_wstat, *d_step_out, *h_step_out; /* h: pinned */
  double surv_per_parent;       /* recent survivors per parent (sizes the next frontier) */
  uint64_t stored_seen;         /* rows in the solution store after the last iteration */
  /* the reference's strategy options (main.c:51-130): -o order, -f prefer failing, restart on a better solution */
  int order, prefer_failing, restart_on_improvement, fail_var_known;
  int *d_prio; /* [n] failure counts (prefer failing) */
  int burst_no_eval;   /* device-driven iterations launch no root evaluation: see enqueue_burst */
  cs_search_switches sw;
  cs_path path;        /* plan_path's answer, kept up to date by create and the setters it depends on */
  /* the solution stream (csgpu_search_set_solution_stream): a ring of [stream_cap][n] int32 rows.  stream_head = the
   * position of the oldest waiting row (= counters[C_STREAM_HEAD]), stream_rows = the host's count of waiting rows,
   * exact whenever no accept is pending (the device's next position is counters[C_STREAM]).  stream_failed: a kernel
   * found no room (CSGPU_E_LIMIT); the stream serves nothing more until csgpu_search_reset */
  int32_t *d_stream;
  int64_t stream_cap, stream_rows, stream_head;
  int stream_failed;
};

extern "C" int csgpu_internal_set_error(int code, const char *msg); /* cs_capi.hip */
static int fail(int code, const char *msg) { return csgpu_internal_set_error(code, msg); }
static int flush_accept_results(csgpu_search *s);

#define HIP_OK(expr)                                                           \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess) return fail(CSGPU_E_HIP, hipGetErrorString(e_));     \
  } while (0)
#define TRY(expr)                                                              \
  do {                                                                         \
    const int rc_ = (expr);                                                    \
    if (rc_ != CSGPU_OK) return rc_;                                           \
  } while (0)

/* the path follows from the objective, the model, the strategy, the switches and the iteration sizes */
static cs_path plan_path(const csgpu_search *s) {
  const int default_rule = s->order == 1 && !s->prefer_failing; /* the only one the level kernels implement */
  if (s->objective == CS_OBJ_ALL)
    return csgpu_internal_step_kind(s->m) != 0 && !s->sw.fused_off && !s->sw.eval_always && default_rule ? PATH_LEVELS
                                                                                                          : PATH_HOST;
  /* ANY dives with few parents and must see the accept before it decides: one workgroup */
  const int split = s->sw.burst_split && s->objective != CS_OBJ_ANY;
  const int64_t most = split ? BURST_PARENTS_MAX : SMALL_PARENTS;
  if (s->sw.burst_off || s->parents_max > most || s->parents_max * s->max_width > s->max_children) return PATH_HOST;
  return split ? PATH_BURST_SPLIT : PATH_BURST_ONE;
}

static int burst_path(const csgpu_search *s) { return s->path == PATH_BURST_ONE || s->path == PATH_BURST_SPLIT; }

/* the sense of cs_objective_bound: 1 minimise, 2 maximise, 0 neither */
static int objective_sense(int objective) { return objective == CS_OBJ_MIN ? 1 : (objective == CS_OBJ_MAX ? 2 : 0); }

/* pool rows an iteration keeps free above its survivors: n_vars * max_width, what a depth-first walk of one parent per
 * iteration can add; the room limit is the capacity below that reserve (all of it, for a pool smaller than that) */
static int64_t pool_reserve(const csgpu_search *s) { return (int64_t)s->n * s->max_width; }
static int64_t pool_room_limit(const csgpu_search *s) { return s->cap > pool_reserve(s) ? s->cap - pool_reserve(s) : s->cap; }

/* survivors per workgroup of cs_scatter: about 4096 state elements per workgroup, fewer when that would leave most of
 * the machine idle with `children` children */
static int scatter_cpb(int n, int64_t children) {
  int cpb = 4096 / n;
  cpb = cpb < 4 ? 4 : (cpb > SB ? SB : cpb);
  while (cpb > 4 && children / cpb < 2048) cpb >>= 1;
  return cpb;
}

/* cs_branch<S> / cs_emit<S>: 16, 32 or 64 lanes per parent; `launch` is called with S as a std::integral_constant */
template <typename F> static void launch_seg(int n, F launch) {
  if (n <= 16) launch(std::integral_constant<int, 16>());
  else if (n <= 32) launch(std::integral_constant<int, 32>());
  else launch(std::integral_constant<int, 64>());
}

/* the captured burst holds the branching rule, the incumbent pointer and the stream's arguments: whatever changes them
 * drops it, and the next burst captures it again */
static void drop_burst_graph(csgpu_search *s) {
  if (s->burst_exec != NULL) (void)hipGraphExecDestroy(s->burst_exec);
  s->burst_exec = NULL;
}

extern "C" void csgpu_search_free(csgpu_search *s) {
  if (s == NULL) return;
  if (s->borrowers > 0) { /* other engines' kernels and graphs still write the incumbent word in s->d_counters */
    s->free_pending = 1;
    return;
  }
  if (s->lender != NULL) {
    csgpu_search *l = s->lender;
    s->lender = NULL;
    if (--l->borrowers == 0 && l->free_pending) csgpu_search_free(l);
  }
  (void)hipSetDevice(s->device);
  if (s->counted) csgpu_internal_engine_ref(s->m, -1);
  (void)hipFree(s->pool_forb); (void)hipFree(s->d_child_forb); (void)hipFree(s->d_rebuild_nodes);
  (void)hipFree(s->pool); (void)hipFree(s->d_choice); (void)hipFree(s->d_child_off); (void)hipFree(s->d_block_sum); (void)hipFree(s->d_block_skip);
  (void)hipFree(s->d_nodes); (void)hipFree(s->d_child_states); (void)hipFree(s->d_complete_states);
  (void)hipFree(s->d_results); (void)hipFree(s->d_dest); (void)hipFree(s->d_complete_list); (void)hipFree(s->d_truth);
  (void)hipFree(s->d_block_surv); (void)hipFree(s->d_block_comp); (void)hipFree(s->d_surv_off); (void)hipFree(s->d_comp_off);
  (void)hipFree(s->d_block_cuts); (void)hipFree(s->d_block_props); (void)hipFree(s->d_block_revs);
  (void)hipFree(s->d_counters); (void)hipFree(s->d_solutions);
  (void)hipFree(s->seed);
  (void)hipFree(s->d_best_solution);
  (void)hipFree(s->d_burst);
  (void)hipFree(s->d_prio);
  (void)hipFree(s->d_stream);
  (void)hipFree(s->d_fill); (void)hipFree(s->d_ticket); (void)hipFree(s->d_wstat); (void)hipFree(s->d_step_out);
  if (s->h_step_out) (void)hipHostFree(s->h_step_out);
  if (s->h_burst) (void)hipHostFree(s->h_burst);
  drop_burst_graph(s);
  if (s->burst_stream) (void)hipStreamDestroy(s->burst_stream);
  free(s);
}

/* the rest of csgpu_search_create, on an engine whose sizes are checked: what follows from the model and the switches,
 * and the buffers.  A failure leaves the engine to csgpu_search_free. */
static int search_init(csgpu_search *s) {
  const csgpu_model *m = s->m;
  const int n = s->n;
  const int64_t max_children = s->max_children;
  s->sw = read_switches();
  s->objective = csgpu_model_objective(m);
  s->obj_var = csgpu_model_objective_var(m);
  s->max_parents = max_children / s->max_width;
  /* ALL walks the whole tree anyway: widest batches.  ANY/MIN/MAX profit from going deep first
   * (a first solution / a good incumbent early prunes everything else), so only the newest 64
   * open states are expanded per iteration. */
  s->avg_children = (double)s->max_width;
  s->parents_limit = s->objective == CS_OBJ_ALL ? s->max_parents : 64;
  if (s->parents_limit > s->max_parents) s->parents_limit = s->max_parents;
  s->parents_max = s->parents_limit;
  if (s->objective == CS_OBJ_MIN || s->objective == CS_OBJ_MAX) { /* ANY stays depth-first */
    /* parents of a device-driven MIN / MAX iteration once the pool holds a backlog (tuning: CSGPU_SEARCH_PARENTS_MAX) */
    /* schedule-12 MIN: 9.7 s with 256, 7.3 s with 512, 6.3 s with 1,024 (round 3, single-workgroup bookkeeping); with the
     * bookkeeping over many workgroups 3.84 s with 1,024 and 3.37 s with 2,048 (10 % more nodes in 20 % fewer, fuller
     * iterations).  What holds an iteration down after that is the share of the pool it takes -- a sixteenth of it was
     * rarely 2,048 states -- and the child buffer (parents x widest interval must fit): with a QUARTER of the pool per
     * iteration schedule-12 takes 2.30 s at 2,048 parents, 1.80 s at 4,096 (2^20 children), 1.68 s at 8,192 (2^21;
     * 1.53e9 nodes in 11,001 iterations of 150 us: the fixpoint kernel at its throughput) and 1.87 s at 16,384 -- from
     * there on the nodes the breadth costs (2.1e9) outweigh the launches it saves */
    int64_t want = s->sw.parents_max; /* 8,192 by default: see B_BACKLOG_DIV in run_burst */
    const int64_t most = s->sw.burst_split ? BURST_PARENTS_MAX : SMALL_PARENTS; /* what one workgroup scans */
    if (want > most) want = most;
    s->parents_max = want < s->max_parents ? want : s->max_parents;
    if (s->parents_max < s->parents_limit) s->parents_max = s->parents_limit;
  }
  s->max_solutions = 1024;
  s->restart_base = s->objective == CS_OBJ_ANY ? 64 : 0;
  s->order = 1;
  s->holes.order = 1;
  s->holes.prio = NULL;
  s->holes.pool_forb = NULL;
  s->holes.root_lo = csgpu_internal_root_lo(m);
  s->path = plan_path(s);
  const int levels = s->path == PATH_LEVELS;
  const size_t row = (size_t)n * sizeof(cs_val);
#define ALLOC(ptr, bytes) HIP_OK(hipMalloc((void **)&(ptr), (bytes)))
  ALLOC(s->pool, row * (size_t)s->cap);
  /* CSGPU_SEARCH_SETS=0: interval rows only in the pool of the separate-kernel path too (the fixpoints then run on
   * kernel 7 / kernel 5's rebuild entry, and no child is cut without a launch); the level kernels keep none either */
  s->fw = s->obj_var < 0 && !s->sw.sets_off && !levels ? csgpu_model_forbidden_words(m) : 0;
  s->stage_rows = max_children;
  if (levels) {
    /* twice the rows a frontier's children may have: a wave's region then takes the worst case of a ticket of 64 parents
     * (fewer parents per ticket and the ticket counter limits the launch, cs_capi.hip; CSGPU_STEP_STAGE_MULT tunes it) */
    s->stage_rows = max_children * s->sw.stage_mult;
    /* one wave per parent (33 to 256 variables): room for the children of four parents in every wave's region */
    if (s->stage_rows < csgpu_internal_step_stage_rows(m)) s->stage_rows = csgpu_internal_step_stage_rows(m);
    if (s->stage_rows > s->cap) s->stage_rows = s->cap;
  }
  if (levels) { /* interval rows only: no sets in the pool, nothing to rebuild for states put from outside */
    const int64_t waves = csgpu_internal_step_waves(m);
    ALLOC(s->d_fill, sizeof(uint32_t) * (size_t)waves);
    ALLOC(s->d_wstat, sizeof(uint64_t) * 8 * (size_t)waves);
    ALLOC(s->d_ticket, 1024); /* sixteen counters on their own 64-byte lines */
    ALLOC(s->d_step_out, sizeof(uint64_t) * 8);
    HIP_OK(hipHostMalloc((void **)&s->h_step_out, sizeof(uint64_t) * 8, 0));
  }
  if (s->fw > 0) {
    ALLOC(s->pool_forb, (size_t)n * s->fw * 8 * (size_t)s->cap);
    ALLOC(s->d_child_forb, (size_t)n * s->fw * 8 * (size_t)max_children);
    ALLOC(s->d_rebuild_nodes, sizeof(csgpu_node) * (size_t)max_children);
  }
  /* up to max_children / 2 parents when every parent has two children */
  ALLOC(s->d_choice, sizeof(cs_choice) * (size_t)max_children);
  ALLOC(s->d_child_off, sizeof(int) * ((size_t)max_children + 1));
  ALLOC(s->d_block_sum, sizeof(int) * ((size_t)max_children + 1));
  ALLOC(s->d_block_skip, sizeof(int) * ((size_t)max_children + 1));
  ALLOC(s->d_nodes, sizeof(csgpu_node) * (size_t)max_children);
  ALLOC(s->d_child_states, row * (size_t)(levels ? s->stage_rows : max_children));
  if (!levels) ALLOC(s->d_complete_states, row * (size_t)max_children);
  ALLOC(s->d_results, sizeof(csgpu_result) * (size_t)max_children);
  ALLOC(s->d_dest, sizeof(int) * (size_t)max_children);
  ALLOC(s->d_complete_list, sizeof(int) * (size_t)max_children);
  ALLOC(s->d_truth, sizeof(int) * (size_t)max_children);
  {
    size_t blocks = ((size_t)max_children + SB - 1) / SB + 1;
    if (blocks < BURST_CLASS_WGS) blocks = BURST_CLASS_WGS;
    ALLOC(s->d_block_surv, sizeof(int) * blocks);
    ALLOC(s->d_block_comp, sizeof(int) * blocks);
    ALLOC(s->d_block_cuts, sizeof(int) * blocks);
    ALLOC(s->d_block_props, sizeof(int) * blocks);
    ALLOC(s->d_block_revs, sizeof(int) * blocks);
    ALLOC(s->d_surv_off, sizeof(int) * (blocks + 1));
    ALLOC(s->d_comp_off, sizeof(int) * (blocks + 1));
  }
  ALLOC(s->d_counters, sizeof(unsigned long long) * C_COUNT);
  s->d_best = (int *)(s->d_counters + C_BEST);
  ALLOC(s->d_solutions, sizeof(int32_t) * (size_t)n * (size_t)s->max_solutions);
  ALLOC(s->d_best_solution, sizeof(int32_t) * (size_t)n);
  if (s->fw == 1 && s->holes.root_lo != NULL && !s->sw.holes_off) s->holes.pool_forb = s->pool_forb;
  ALLOC(s->d_burst, sizeof(unsigned long long) * B_COUNT);
#undef ALLOC
  HIP_OK(hipHostMalloc((void **)&s->h_burst, sizeof(unsigned long long) * (B_COUNT + C_COUNT + 1), 0));
  HIP_OK(hipStreamCreate(&s->burst_stream));
  int64_t info[8];
  s->burst_no_eval = !s->sw.eval_always && csgpu_model_device_info(m, info) == CSGPU_OK && info[2] == 0;
  return csgpu_search_reset(s); /* the starting statistics, incumbent and counters */
}

extern "C" int csgpu_search_create(const csgpu_model *m, int64_t pool_capacity, int64_t max_children,
                                   csgpu_search **out) {
  if (m == NULL || out == NULL || pool_capacity < 1 || max_children < 1) return fail(CSGPU_E_ARG, "bad argument");
  const int n = csgpu_model_num_vars(m);
  if (n <= 0) return fail(CSGPU_E_ARG, "model without variables");
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return fail(CSGPU_E_HIP, "hipGetDevice");
  /* widest root interval bounds the branching factor (domains only shrink below the root) */
  csgpu_val *dom = (csgpu_val *)malloc((size_t)n * sizeof *dom);
  if (dom == NULL) return fail(CSGPU_E_LIMIT, "out of memory");
  csgpu_model_get_domains(m, dom);
  /* children of one parent: the interval's values if it has at most SPLIT_WIDTH of them, else 2.
   * A wide root interval gets narrow by halving, so SPLIT_WIDTH bounds every variable that
   * starts wider than that. */
  int64_t max_width = 2;
  for (int v = 0; v < n; v++) {
    int64_t w = (int64_t)dom[v].hi - (int64_t)dom[v].lo + 1;
    if (w > SPLIT_WIDTH) w = SPLIT_WIDTH;
    if (w > max_width) max_width = w;
  }
  free(dom);
  if (max_children < max_width) max_children = max_width;
  if (max_children > 0x3fffffff) return fail(CSGPU_E_LIMIT, "max_children too large");
  if (pool_capacity < max_children + 1) pool_capacity = max_children + 1;
  if (pool_capacity > 0x7fffffff) return fail(CSGPU_E_LIMIT, "pool_capacity too large");
  csgpu_search *s = (csgpu_search *)calloc(1, sizeof *s);
  if (s == NULL) return fail(CSGPU_E_LIMIT, "out of memory");
  s->m = m;
  s->n = n;
  s->device = device;
  s->max_width = max_width;
  s->max_children = max_children;
  s->cap = pool_capacity;
  csgpu_internal_engine_ref(m, 1);
  s->counted = 1;
  const int rc = search_init(s);
  if (rc != CSGPU_OK) {
    csgpu_search_free(s);
    return rc;
  }
  *out = s;
  return CSGPU_OK;
}

static int search_put(csgpu_search *s, const csgpu_val *d_states, int64_t count);

extern "C" int csgpu_search_put(csgpu_search *s, const csgpu_val *d_states, int64_t count) {
  if (s == NULL || (count > 0 && d_states == NULL) || count < 0) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  const auto t0 = std::chrono::steady_clock::now();
  int rc = search_put(s, d_states, count);
  if (rc == CSGPU_OK && count > 0) {
    HIP_OK(hipDeviceSynchronize()); /* the rebuild launches are part of the cost */
    s->put_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    s->put_states += count;
  }
  return rc;
}

extern "C" int csgpu_search_put_cost(const csgpu_search *s, double *seconds, int64_t *states) {
  if (s == NULL || seconds == NULL || states == NULL) return fail(CSGPU_E_ARG, "bad argument");
  *seconds = s->put_seconds;
  *states = s->put_states;
  return CSGPU_OK;
}

static int search_put(csgpu_search *s, const csgpu_val *d_states, int64_t count) {
  if (s->top + count > s->cap) return fail(CSGPU_E_LIMIT, "state pool is full");
  if (count > 0)
    HIP_OK(hipMemcpy(s->pool + (size_t)s->top * s->n, d_states, (size_t)count * s->n * sizeof(cs_val),
                     hipMemcpyDeviceToDevice));
  if (count > 0 && s->path == PATH_LEVELS) /* the pool of the fused path holds engine rows (cs_step.hip.h) */
    TRY(csgpu_internal_step_import(s->m, (csgpu_val *)s->pool, s->top, count, NULL));
  if (count > 0 && s->fw > 0) {
    /* states arriving from outside (the root, another rank) carry no sets: rebuild them in place,
     * max_children rows at a time (the batch buffers are free between iterations) */
    for (int64_t done = 0; done < count; done += s->max_children) {
      const int64_t k = count - done < s->max_children ? count - done : s->max_children;
      hipLaunchKernelGGL(cs_fill_rebuild, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, 0, s->d_rebuild_nodes,
                         (long long)(s->top + done), (int)k);
      TRY(csgpu_propagate_batch_fb(s->m, (const csgpu_val *)s->pool, NULL, s->d_rebuild_nodes,
                                   (csgpu_val *)s->d_child_states, (uint64_t *)s->d_child_forb, s->d_results, k,
                                   NULL));
      HIP_OK(hipMemcpy(s->pool_forb + (size_t)(s->top + done) * s->n * s->fw, s->d_child_forb,
                       (size_t)k * s->n * s->fw * 8, hipMemcpyDeviceToDevice));
    }
  }
  if (count > 0 && (s->restart_base > 0 || s->restart_on_improvement) && !s->st.iterations) {
    /* remember what the search was started from (only states put before the first iteration) */
    if (s->seed_count + count > s->seed_cap) {
      const int64_t cap = (s->seed_count + count) * 2;
      cs_val *grown = NULL;
      HIP_OK(hipMalloc((void **)&grown, (size_t)cap * s->n * sizeof(cs_val)));
      if (s->seed_count > 0)
        HIP_OK(hipMemcpy(grown, s->seed, (size_t)s->seed_count * s->n * sizeof(cs_val), hipMemcpyDeviceToDevice));
      (void)hipFree(s->seed);
      s->seed = grown;
      s->seed_cap = cap;
    }
    HIP_OK(hipMemcpy(s->seed + (size_t)s->seed_count * s->n, d_states, (size_t)count * s->n * sizeof(cs_val),
                     hipMemcpyDeviceToDevice));
    s->seed_count += count;
  }
  s->top += count;
  if (s->top > s->peak) s->peak = s->top;
  return CSGPU_OK;
}

extern "C" int csgpu_search_reset(csgpu_search *s) {
  if (s == NULL) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  s->top = 0;
  s->peak = 0;
  memset(&s->st, 0, sizeof s->st);
  s->st.best = s->objective == CS_OBJ_MIN ? CS_DOM_MAX : (s->objective == CS_OBJ_MAX ? CS_DOM_MIN : 0); /* no solution yet */
  s->seed_count = 0;
  s->since_restart = 0;
  s->luby_threshold = 1;
  s->luby_counter = 1;
  s->put_seconds = 0.0;
  s->put_states = 0;
  s->have_best_solution = 0;
  s->pending_complete = 0;
  s->surv_per_parent = (double)s->max_width;
  s->stored_seen = 0;
  s->stream_rows = 0; /* the counters below hold the device's positions: the stream is empty and stays on */
  s->stream_head = 0;
  s->stream_failed = 0;
  if (s->d_prio != NULL) HIP_OK(hipMemset(s->d_prio, 0, sizeof(int) * (size_t)s->n));
  HIP_OK(hipMemset(s->d_counters, 0, sizeof(unsigned long long) * C_COUNT));
  HIP_OK(hipMemcpy(s->d_best, &s->st.best, sizeof(int), hipMemcpyHostToDevice));
  return CSGPU_OK;
}

extern "C" int csgpu_search_put_host(csgpu_search *s, const csgpu_val *states, int64_t count) {
  if (s == NULL || (count > 0 && states == NULL) || count < 0) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  if (count == 0) return CSGPU_OK;
  cs_val *tmp = NULL;
  const size_t bytes = (size_t)count * s->n * sizeof(cs_val);
  HIP_OK(hipMalloc((void **)&tmp, bytes));
  hipError_t e = hipMemcpy(tmp, states, bytes, hipMemcpyHostToDevice);
  int rc = e == hipSuccess ? csgpu_search_put(s, (const csgpu_val *)tmp, count) : fail(CSGPU_E_HIP, hipGetErrorString(e));
  (void)hipFree(tmp);
  return rc;
}

extern "C" int csgpu_search_set_restart(csgpu_search *s, int64_t iterations) {
  if (s == NULL || iterations < 0) return fail(CSGPU_E_ARG, "bad argument");
  s->restart_base = s->objective == CS_OBJ_ANY ? iterations : 0;
  return CSGPU_OK;
}

extern "C" int csgpu_search_set_strategy(csgpu_search *s, int order, int prefer_failing) {
  if (s == NULL || order < 0 || order > 4) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  if (s->top != 0 || s->st.iterations != 0) return fail(CSGPU_E_STATE, "the strategy is set before the first state is put");
  const int is_default = order == 1 && !prefer_failing;
  if (!is_default) {
    /* the level kernels and the cut of children by the parent's own set implement the default rule only; a count of
     * failures needs the emptied variable of a failing child, which the interval kernels report */
    s->fw = 0;
    s->holes.pool_forb = NULL;
  }
  s->order = order;
  s->prefer_failing = prefer_failing != 0;
  s->path = plan_path(s);
  s->holes.order = order;
  s->holes.prio = NULL;
  if (s->prefer_failing) {
    if (s->d_prio == NULL) HIP_OK(hipMalloc((void **)&s->d_prio, sizeof(int) * (size_t)s->n));
    HIP_OK(hipMemset(s->d_prio, 0, sizeof(int) * (size_t)s->n));
    s->holes.prio = s->d_prio;
    const int k = csgpu_model_get_kernel(s->m);
    s->fail_var_known = k == 1 || k == 6 || k == 7;
  }
  drop_burst_graph(s); /* the graph holds the old rule */
  return CSGPU_OK;
}

extern "C" int csgpu_search_set_restart_on_improvement(csgpu_search *s, int on) {
  if (s == NULL) return fail(CSGPU_E_ARG, "bad argument");
  if (s->top != 0 || s->st.iterations != 0) return fail(CSGPU_E_STATE, "set before the first state is put");
  s->restart_on_improvement = on != 0 && (s->objective == CS_OBJ_MIN || s->objective == CS_OBJ_MAX);
  return CSGPU_OK;
}

extern "C" int csgpu_search_take(csgpu_search *s, csgpu_val *d_states, int64_t max, int64_t *count) {
  if (s == NULL || d_states == NULL || count == NULL || max < 0) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  int64_t k = max < s->top ? max : s->top;
  *count = k;
  if (k == 0) return CSGPU_OK;
  HIP_OK(hipMemcpy(d_states, s->pool, (size_t)k * s->n * sizeof(cs_val), hipMemcpyDeviceToDevice));
  if (s->path == PATH_LEVELS) { /* engine rows -> interval rows, in the caller's buffer */
    TRY(csgpu_internal_step_export(s->m, d_states, 0, k, NULL));
    HIP_OK(hipDeviceSynchronize());
  }
  /* fill the hole at the bottom with the newest rows */
  const int64_t rest = s->top - k, mv = rest < k ? rest : k;
  if (mv > 0) {
    hipLaunchKernelGGL(cs_move_rows, dim3((unsigned)((mv + 3) / 4)), dim3(SB), 0, 0, (unsigned long long *)s->pool,
                       (long long)(s->top - mv), 0ll, (int)mv, s->n);
    if (s->fw > 0)
      hipLaunchKernelGGL(cs_move_rows, dim3((unsigned)((mv + 3) / 4)), dim3(SB), 0, 0, s->pool_forb,
                         (long long)(s->top - mv), 0ll, (int)mv, s->n * s->fw);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
  }
  s->top -= k;
  return CSGPU_OK;
}

extern "C" int csgpu_search_take_host(csgpu_search *s, csgpu_val *states, int64_t max, int64_t *count) {
  if (s == NULL || states == NULL || count == NULL || max < 0) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  const int64_t k = max < s->top ? max : s->top;
  *count = 0;
  if (k == 0) return CSGPU_OK;
  cs_val *tmp = NULL;
  const size_t bytes = (size_t)k * s->n * sizeof(cs_val);
  HIP_OK(hipMalloc((void **)&tmp, bytes));
  int64_t got = 0;
  int rc = csgpu_search_take(s, (csgpu_val *)tmp, k, &got);
  if (rc == CSGPU_OK) {
    const hipError_t e = hipMemcpy(states, tmp, (size_t)got * s->n * sizeof(cs_val), hipMemcpyDeviceToHost);
    if (e == hipSuccess) *count = got;
    else rc = fail(CSGPU_E_HIP, hipGetErrorString(e));
  }
  (void)hipFree(tmp);
  return rc;
}

extern "C" int csgpu_internal_search_info(const csgpu_search *s, int *objective, int *obj_var, int *n_vars,
                                          int *restarts, int64_t *stream_rows) {
  if (s == NULL) return CSGPU_E_ARG;
  if (objective != NULL) *objective = s->objective;
  if (obj_var != NULL) *obj_var = s->obj_var;
  if (n_vars != NULL) *n_vars = s->n;
  if (restarts != NULL) *restarts = s->restart_base > 0 || s->restart_on_improvement;
  if (stream_rows != NULL) *stream_rows = s->d_stream != NULL ? s->stream_cap : 0;
  return CSGPU_OK;
}

extern "C" int csgpu_search_set_parents(csgpu_search *s, int64_t parents_per_iteration) {
  if (s == NULL || parents_per_iteration < 1) return fail(CSGPU_E_ARG, "bad argument");
  const int64_t limit = parents_per_iteration < s->max_parents ? parents_per_iteration : s->max_parents;
  if ((s->lender != NULL || s->borrowers > 0) && (limit > SMALL_PARENTS || limit * s->max_width > s->max_children))
    return fail(CSGPU_E_STATE, "engines that share an incumbent run device-driven iterations: at most 1,024 parents per iteration");
  s->parents_limit = limit;
  s->parents_max = s->parents_limit; /* an explicit setting is taken literally */
  s->path = plan_path(s);
  return CSGPU_OK;
}

extern "C" int csgpu_search_set_best(csgpu_search *s, int32_t best) {
  if (s == NULL) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  TRY(flush_accept_results(s)); /* an unread incumbent of the last iteration must not be overwritten */
  int better = (s->objective == CS_OBJ_MIN && best < s->st.best) || (s->objective == CS_OBJ_MAX && best > s->st.best);
  if (better) {
    s->st.best = best;
    HIP_OK(hipMemcpy(s->d_best, &best, sizeof(int), hipMemcpyHostToDevice));
  }
  return CSGPU_OK;
}

extern "C" int csgpu_search_set_solution_stream(csgpu_search *s, int64_t rows) {
  if (s == NULL) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  if (s->top != 0 || s->st.iterations != 0) return fail(CSGPU_E_STATE, "the solution stream is set before the first state is put");
  if (s->lender != NULL || s->borrowers > 0)
    return fail(CSGPU_E_STATE, "an engine that shares its incumbent has no solution stream");
  /* one parent's children at most per row of room: the rule by which an iteration is sized (stream_room) */
  if (rows < s->max_width || rows > 0x7fffffff) return fail(CSGPU_E_ARG, "solution stream rows out of range");
  if (s->d_stream != NULL && s->stream_cap != rows) {
    (void)hipFree(s->d_stream);
    s->d_stream = NULL;
  }
  if (s->d_stream == NULL) HIP_OK(hipMalloc((void **)&s->d_stream, (size_t)rows * s->n * sizeof(int32_t)));
  s->stream_cap = rows;
  s->stream_rows = 0;
  s->stream_head = 0;
  s->stream_failed = 0;
  HIP_OK(hipMemset(s->d_counters + C_STREAM, 0, sizeof(unsigned long long) * 3)); /* C_STREAM, C_STREAM_HEAD, C_STREAM_ERR */
  drop_burst_graph(s); /* the graph holds the old arguments */
  return CSGPU_OK;
}

/* rows of the stream that are free for what the coming iterations append: the accept that is still unread counts with
 * what it may add (ALL: every complete child of its iteration; otherwise one row) */
static int64_t stream_room(const csgpu_search *s) {
  const int64_t pending = s->objective == CS_OBJ_ALL ? s->pending_complete : (s->pending_complete > 0 ? 1 : 0);
  return s->stream_cap - s->stream_rows - pending;
}

extern "C" int csgpu_search_share_incumbent(csgpu_search *s, csgpu_search *with) {
  if (s == NULL || with == NULL || s->objective != with->objective || s->obj_var != with->obj_var)
    return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  if (s->d_stream != NULL || with->d_stream != NULL)
    return fail(CSGPU_E_STATE, "an engine with a solution stream does not share its incumbent");
  if (s->objective != CS_OBJ_MIN && s->objective != CS_OBJ_MAX) return CSGPU_OK; /* nothing to share */
  if (!burst_path(s) || !burst_path(with))
    return fail(CSGPU_E_STATE, "a shared incumbent needs the device-driven iterations");
  TRY(flush_accept_results(s));
  /* the better of the two goes into the shared word */
  int mine = 0, theirs = 0;
  HIP_OK(hipMemcpy(&mine, s->d_best, sizeof(int), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(&theirs, with->d_best, sizeof(int), hipMemcpyDeviceToHost));
  const int best = s->objective == CS_OBJ_MIN ? (mine < theirs ? mine : theirs) : (mine > theirs ? mine : theirs);
  HIP_OK(hipMemcpy(with->d_best, &best, sizeof(int), hipMemcpyHostToDevice));
  if (s == with || s->lender == with) return CSGPU_OK;
  if (s->borrowers > 0) return fail(CSGPU_E_STATE, "an engine whose incumbent word is shared by others cannot borrow one itself");
  csgpu_search *owner = with->lender != NULL ? with->lender : with; /* chains collapse onto the engine that owns the word */
  if (s->lender != NULL && --s->lender->borrowers == 0 && s->lender->free_pending) csgpu_search_free(s->lender);
  s->lender = owner;
  owner->borrowers++;
  s->d_best = owner->d_best;
  s->st.best = best;
  s->path = plan_path(s);
  drop_burst_graph(s); /* the graph holds the old pointer */
  return CSGPU_OK;
}

/* the accept kernel's results, read one host round trip later than they were produced */
static int apply_accept_results(csgpu_search *s, unsigned long long solutions_total, int best) {
  if (s->pending_complete == 0) return CSGPU_OK;
  const int improved = (s->objective == CS_OBJ_MIN || s->objective == CS_OBJ_MAX) && solutions_total > s->st.solutions &&
                       best != s->st.best;
  /* ALL / ANY: every accepted solution went to the stream; MIN / MAX: the pick below goes there */
  if (s->d_stream != NULL && (s->objective == CS_OBJ_ALL || s->objective == CS_OBJ_ANY))
    s->stream_rows += (int64_t)(solutions_total - s->st.solutions);
  s->st.solutions = solutions_total;
  if (improved) {
    /* the complete children and their truth values of that iteration are still in place */
    hipLaunchKernelGGL(cs_pick_best, dim3(1), dim3(64), 0, 0, s->d_complete_states, s->d_truth, (int)s->pending_complete,
                       s->n, s->objective, s->obj_var, best, s->d_best_solution, s->d_stream, (long long)s->stream_cap,
                       s->d_counters);
    if (s->d_stream != NULL) s->stream_rows++;
    s->have_best_solution = 1;
    s->best_solution_value = best;
  }
  if (s->objective == CS_OBJ_MIN || s->objective == CS_OBJ_MAX) s->st.best = best;
  s->pending_complete = 0;
  HIP_OK(hipGetLastError());
  return CSGPU_OK;
}

static int flush_accept_results(csgpu_search *s) {
  if (s->pending_complete == 0) return CSGPU_OK;
  unsigned long long tail[C_COUNT - C_SOLUTIONS];
  HIP_OK(hipMemcpy(tail, s->d_counters + C_SOLUTIONS, sizeof tail, hipMemcpyDeviceToHost));
  return apply_accept_results(s, tail[0], (int)(unsigned)tail[C_BEST - C_SOLUTIONS]);
}

/* ALL on a model with a step kernel: the newest `parents` rows of the pool are one frontier, expanded by one launch.
 * How many: as many as the pool and the staging buffer are likely to have room for the survivors of (the recent
 * survivors per parent size the attempt; a wave that could overflow its region stops drawing parents and the
 * undrawn ones stay where they are, so a wrong guess costs time, never a state). */
static int one_iteration_fused(csgpu_search *s) {
  const int64_t reserve = pool_reserve(s);
  const double spp = s->surv_per_parent < 0.25 ? 0.25 : s->surv_per_parent;
  int64_t parents = s->top;
  /* staging: expect spp survivors per parent, keep a factor of two in hand */
  const int64_t by_stage = (int64_t)((double)s->stage_rows / (2.0 * spp));
  if (parents > by_stage) parents = by_stage;
  /* pool: a depth-first walk in batches of P holds about P * spp rows per level that is still open below the
   * frontier (at most n levels); leave that much room, shrink P as the pool fills */
  const int64_t room = s->cap - s->top - reserve;
  const int64_t by_pool = room > 0 ? (int64_t)((double)room / (spp * (double)s->n)) : 0;
  if (parents > by_pool) parents = by_pool;
  if (parents > 0x3fffffff) parents = 0x3fffffff;
  if (parents < 1) parents = 1;
  /* the solution stream: a parent has at most max_width children, so room / max_width parents cannot overflow it
   * (csgpu_search_run has seen to room >= max_width) */
  if (s->d_stream != NULL && parents > stream_room(s) / s->max_width) parents = stream_room(s) / s->max_width;
  /* (no worst-case test "every child of every parent survives": the staging rows handed to the launch below are
   * capped by what the pool has room for, and a wave whose region could overflow stops drawing parents) */
  if (s->top - 1 + s->max_width > s->cap) return fail(CSGPU_E_LIMIT, "state pool is full");
  csgpu_step_launch L;
  L.pool = (const csgpu_val *)s->pool;
  L.first_row = s->top - parents;
  L.parents = (int32_t)parents;
  L.stage = (csgpu_val *)s->d_child_states;
  L.stage_rows = s->stage_rows;
  /* the survivors land behind the undrawn parents: never more than the pool has room for above its top (the rows the
   * drawn parents free come on top of that) */
  if (L.stage_rows > s->cap - s->top) L.stage_rows = s->cap - s->top;
  {
    const int64_t limit = csgpu_internal_step_parents_limit(s->m, L.stage_rows);
    if (limit < 1) return fail(CSGPU_E_LIMIT, "state pool is full");
    if (parents > limit) {
      parents = limit;
      L.first_row = s->top - parents;
      L.parents = (int32_t)parents;
    }
  }
  L.fill = s->d_fill;
  L.wstat = s->d_wstat;
  L.ticket = s->d_ticket;
  L.out = s->d_step_out;
  L.solutions = s->d_solutions;
  L.stored = (uint64_t *)(s->d_counters + C_STORED);
  L.max_solutions = s->max_solutions;
  L.store_open = s->stored_seen < (uint64_t)s->max_solutions;
  L.stream = s->d_stream;
  L.stream_base = s->stream_head + s->stream_rows;
  L.stream_limit = s->stream_head + s->stream_cap;
  L.stream_cap = s->stream_cap;
  L.stream_err = (uint64_t *)(s->d_counters + C_STREAM_ERR);
  HIP_OK(hipMemsetAsync(s->d_ticket, 0, 1024, 0));
  TRY(csgpu_internal_step(s->m, &L, NULL));
  HIP_OK(hipMemcpyAsync(s->h_step_out, s->d_step_out, sizeof(uint64_t) * 8, hipMemcpyDeviceToHost, 0));
  HIP_OK(hipStreamSynchronize(0));
  const uint64_t *h = s->h_step_out;
  const int64_t consumed = (int64_t)h[0], survivors = (int64_t)h[1];
  if (consumed < 1) return fail(CSGPU_E_LIMIT, "internal: a frontier of the fused search consumed no parent");
  s->top += survivors - consumed;
  if (s->top > s->peak) s->peak = s->top;
  s->st.iterations++;
  s->st.nodes += h[2];
  s->st.cuts += h[3];
  s->st.props += h[4];
  s->st.revisions += h[5];
  s->st.solutions += h[6];
  if (s->d_stream != NULL) s->stream_rows += (int64_t)h[6];
  s->stored_seen = h[7];
  s->surv_per_parent = 0.5 * s->surv_per_parent + 0.5 * ((double)survivors / (double)consumed);
  if (s->sw.trace)
    fprintf(stderr, "fused: parents %lld consumed %lld survivors %lld top %lld nodes %llu cuts %llu solutions %llu\n",
            (long long)parents, (long long)consumed, (long long)survivors, (long long)s->top, (unsigned long long)h[2],
            (unsigned long long)h[3], (unsigned long long)h[6]);
  return CSGPU_OK;
}

static int one_iteration(csgpu_search *s) {
  if (s->path == PATH_LEVELS) return one_iteration_fused(s);
  const int n = s->n;
  int64_t parents = s->top < s->parents_limit ? s->top : s->parents_limit;
  const int64_t room_limit = pool_room_limit(s);
  /* ALL walks the whole tree: batches as large as the child buffers allow.  How many parents that is depends on
   * how wide they branch, which is only known after cs_branch; the recent average sizes the attempt (the exact
   * count is checked below and the attempt halved if it does not fit). */
  const int adaptive = s->objective == CS_OBJ_ALL && s->parents_limit == s->max_parents;
  if (adaptive) {
    int64_t guess = (int64_t)((double)s->max_children / (s->avg_children * 1.25));
    if (guess > s->max_children / 2) guess = s->max_children / 2;
    /* and as many as the pool is likely to have room for */
    const double per_parent = s->avg_children > 1.5 ? s->avg_children - 1.0 : 0.5;
    const int64_t room = (int64_t)((double)(room_limit - s->top) / (per_parent * 1.25));
    if (guess > room) guess = room;
    if (guess > parents) parents = guess < s->top ? guess : s->top;
  }
  /* the children of p parents need at most p * max_width rows above the top - p that stay.  A nearly full pool
   * takes as many parents as are guaranteed to fit below a reserve of n_vars * max_width rows, and one parent
   * (strict depth-first, which cannot grow the pool by more than that reserve) once the reserve is reached */
  if (!adaptive || parents <= s->max_parents) {
    if (s->top - parents + parents * s->max_width > room_limit) {
      const int64_t fit = s->max_width > 1 ? (room_limit - s->top) / (s->max_width - 1) : parents;
      parents = s->top < 1 ? 0 : (fit < 1 ? 1 : (fit < parents ? fit : parents));
      if (s->top - parents + parents * s->max_width > s->cap) return fail(CSGPU_E_LIMIT, "state pool is full");
    }
  }
  /* the solution stream (ALL): room / max_width parents cannot overflow it (csgpu_search_run has seen to room >= max_width) */
  if (s->d_stream != NULL && s->objective == CS_OBJ_ALL && parents > stream_room(s) / s->max_width)
    parents = stream_room(s) / s->max_width;
  long long first_row = s->top - parents;
  if (parents == 0) return CSGPU_OK;
  const int small = parents <= SMALL_PARENTS && parents <= s->max_parents;
  const int low_last = s->objective == CS_OBJ_MAX ? 0 : 1;
  const unsigned scramble =
      s->objective == CS_OBJ_ANY ? (unsigned)(s->st.iterations * 2654435761ull + 0x9e3779b9u) | 1u : 0u;
  unsigned long long skipped_now = 0; /* large path: children cut without a launch, known with the child count */
  int64_t children;          /* what the launches are sized for */
  const uint64_t *d_children; /* where the real count is, when the host does not know it yet */
  if (small) {
    /* one workgroup expands; nothing is read back before the fixpoint is launched */
    hipLaunchKernelGGL(cs_expand_small, dim3(1), dim3(1024), 0, 0, s->pool, first_row, (int)parents, n, s->d_nodes,
                       s->d_counters, low_last, scramble, s->holes);
    children = parents * s->max_width;
    d_children = (const uint64_t *)(s->d_counters + C_TOTAL_CHILDREN);
  } else {
    unsigned pb;
    for (;;) {
      HIP_OK(hipMemsetAsync(s->d_counters, 0, sizeof(unsigned long long) * C_PER_ITERATION, 0));
      launch_seg(n, [&](auto S) {
        constexpr int ppb = SB / decltype(S)::value;
        pb = (unsigned)((parents + ppb - 1) / ppb);
        hipLaunchKernelGGL(cs_branch<decltype(S)::value>, dim3(pb), dim3(SB), 0, 0, s->pool, first_row, (int)parents, n,
                           s->d_choice, s->d_block_sum, s->holes, s->d_block_skip);
      });
      hipLaunchKernelGGL(cs_scan, dim3(1), dim3(1024), 0, 0, s->d_block_sum, (int)pb, s->d_child_off, s->d_counters,
                         (int)C_TOTAL_CHILDREN, (const int *)s->d_block_skip, (int)C_SKIPPED);
      /* first host read of the iteration: the number of children, and with it what the previous
       * iteration's accept left behind (solutions so far, incumbent) */
      unsigned long long head[C_COUNT - C_TOTAL_CHILDREN];
      HIP_OK(hipMemcpy(head, s->d_counters + C_TOTAL_CHILDREN, sizeof head, hipMemcpyDeviceToHost));
      children = (int64_t)head[0];
      skipped_now = head[C_SKIPPED - C_TOTAL_CHILDREN];
      TRY(apply_accept_results(s, head[C_SOLUTIONS - C_TOTAL_CHILDREN], (int)(unsigned)head[C_BEST - C_TOTAL_CHILDREN]));
      if (adaptive) s->avg_children = 0.5 * s->avg_children + 0.5 * ((double)children / (double)parents);
      /* the exact fit: the child buffers, and the pool rows above the parents that stay */
      const int fits = children <= s->max_children &&
                       (s->top - parents + children <= room_limit || (parents == 1 && s->top - 1 + children <= s->cap));
      if (fits) break;
      if (parents == 1) return fail(CSGPU_E_LIMIT, "state pool is full");
      parents = parents / 2 > 0 ? parents / 2 : 1;
      first_row = s->top - parents;
    }
    d_children = NULL;
    if (children > s->max_children) return fail(CSGPU_E_LIMIT, "internal: more children than the batch buffers hold");
    launch_seg(n, [&](auto S) {
      hipLaunchKernelGGL(cs_emit<decltype(S)::value>, dim3(pb), dim3(SB), 0, 0, first_row, (int)parents,
                         (const cs_choice *)s->d_choice, (const int *)s->d_child_off, s->d_nodes, low_last, scramble);
    });
  }
  s->top -= parents;
  s->st.iterations++;
  if (children == 0) { /* (large path only) every child was cut by its parent's own set */
    s->st.nodes += skipped_now;
    s->st.cuts += skipped_now;
    return CSGPU_OK;
  }

  /* the incumbent (as the large path's first read left it) tightens "<obj>" for every child (objective.c:101-126) */
  const cs_val lim = cs_objective_bound(objective_sense(s->objective), cs_interval(CS_DOM_MIN, CS_DOM_MAX), s->st.best);
  if (s->fw > 0)
    TRY(csgpu_internal_propagate_fb(s->m, (const csgpu_val *)s->pool, (const uint64_t *)s->pool_forb, s->d_nodes,
                                    (csgpu_val *)s->d_child_states, (uint64_t *)s->d_child_forb, s->d_results, children,
                                    d_children, NULL));
  else
    TRY(csgpu_internal_propagate_obj(s->m, (const csgpu_val *)s->pool, s->d_nodes, (csgpu_val *)s->d_child_states,
                                     s->d_results, children, d_children, lim.lo, lim.hi, NULL));
  const unsigned cb = (unsigned)((children + SB - 1) / SB);
  if (s->prefer_failing)
    hipLaunchKernelGGL(cs_prio_update, dim3(cb), dim3(SB), 0, 0, (const csgpu_result *)s->d_results, (const csgpu_node *)s->d_nodes,
                       (int)children, (const unsigned long long *)d_children, n, s->fail_var_known, s->d_prio);
  if (small) {
    hipLaunchKernelGGL(cs_classify_small, dim3(1), dim3(1024), 0, 0, s->d_results, s->d_dest, s->d_complete_list,
                       s->d_counters, (unsigned long long *)NULL);
  } else {
    hipLaunchKernelGGL(cs_classify_count, dim3(cb), dim3(SB), 0, 0, s->d_results, (int)children, s->d_block_surv,
                       s->d_block_comp, s->d_block_cuts, s->d_block_props, s->d_block_revs);
    hipLaunchKernelGGL(cs_scan_classes, dim3(1), dim3(1024), 0, 0, s->d_block_surv, s->d_block_comp, s->d_block_cuts,
                       s->d_block_props, s->d_block_revs, (int)cb, s->d_surv_off, s->d_comp_off, s->d_counters);
    hipLaunchKernelGGL(cs_classify_assign, dim3(cb), dim3(SB), 0, 0, s->d_results, (int)children, s->d_surv_off,
                       s->d_comp_off, s->d_dest, s->d_complete_list);
  }
  {
    const int cpb = scatter_cpb(n, children);
    hipLaunchKernelGGL(cs_scatter, dim3((unsigned)((children + cpb - 1) / cpb)), dim3(SB), 0, 0, s->d_child_states, s->d_dest,
                       s->d_counters, (long long)s->top, n, s->pool, s->d_child_forb, s->pool_forb, s->fw, cpb,
                       (const unsigned long long *)NULL);
  }
  /* the (only, for a small iteration) host read: class counts, the real number of children, and what the
   * previous iteration's accept left behind */
  unsigned long long c[C_COUNT];
  HIP_OK(hipMemcpy(c, s->d_counters, sizeof c, hipMemcpyDeviceToHost));
  if (small) {
    children = (int64_t)c[C_TOTAL_CHILDREN];
    TRY(apply_accept_results(s, c[C_SOLUTIONS], (int)(unsigned)c[C_BEST]));
  }
  s->top += (int64_t)c[C_SURVIVORS];
  if (s->top > s->peak) s->peak = s->top;
  s->st.nodes += (uint64_t)children + c[C_SKIPPED];
  s->st.cuts += c[C_CUTS] + c[C_SKIPPED];
  s->st.props += c[C_PROPS];
  s->st.revisions += c[C_REVS];

  const int64_t complete = (int64_t)c[C_COMPLETE];
  if (complete > 0) {
    if (s->objective == CS_OBJ_ALL) {
      /* evaluated and accepted where they lie, through the list of their child indices.  On a pure != network
       * (the models with forbidden sets, fw > 0) a complete consistent node IS a solution: a clause between two
       * valued variables was revised when the second of them became a value and would have emptied a domain
       * (propagate_eq_false_lr, propagate.c:106-120), and the root's own valued pairs were checked by the root
       * phase -- evaluating the root (eval_wand over every clause, eval.c:233-255) can only say "true" */
      const int *truth = s->fw > 0 && !s->sw.eval_always ? (const int *)NULL : (const int *)s->d_truth;
      if (truth != NULL)
        TRY(csgpu_internal_eval_list(s->m, (const csgpu_val *)s->d_child_states, s->d_complete_list,
                                     (const uint64_t *)(s->d_counters + C_COMPLETE), complete, s->d_truth, NULL));
      hipLaunchKernelGGL(cs_accept, dim3((unsigned)((complete + SB - 1) / SB)), dim3(SB), 0, 0, s->d_child_states,
                         truth, (int)complete, n, s->objective, s->obj_var, s->d_counters, s->d_solutions,
                         (long long)s->max_solutions, (const int *)s->d_complete_list, s->d_stream, (long long)s->stream_cap);
    } else {
      /* MIN / MAX keep the complete children of the iteration together: cs_pick_best looks at them one host
       * round trip later */
      const unsigned gw = (unsigned)((complete + 3) / 4);
      hipLaunchKernelGGL(cs_gather_complete, dim3(gw), dim3(SB), 0, 0, s->d_child_states, s->d_complete_list,
                         (int)complete, n, s->d_complete_states);
      TRY(csgpu_eval_batch(s->m, (const csgpu_val *)s->d_complete_states, s->d_truth, complete, NULL));
      /* ANY: its one solution goes to the stream here; MIN / MAX: the improving row, by cs_pick_best */
      hipLaunchKernelGGL(cs_accept, dim3((unsigned)((complete + SB - 1) / SB)), dim3(SB), 0, 0, s->d_complete_states,
                         s->d_truth, (int)complete, n, s->objective, s->obj_var, s->d_counters, s->d_solutions,
                         (long long)s->max_solutions, (const int *)NULL,
                         s->objective == CS_OBJ_ANY ? s->d_stream : (int32_t *)NULL, (long long)s->stream_cap);
    }
    /* what accept found is read together with the next iteration's child count (or at the end of the
     * run); ANY stops on the first solution, so it looks at once */
    s->pending_complete = complete;
    if (s->objective == CS_OBJ_ANY) TRY(flush_accept_results(s));
  }
  HIP_OK(hipGetLastError());
  return CSGPU_OK;
}

/* ---- device-driven iterations (ANY / MIN / MAX) ----
 * These searches expand a few parents per iteration (depth first towards a solution / a better incumbent), so an
 * iteration is a handful of small launches and, driven from the host, mostly the round trip for its counts.
 * Here BURST_ITERATIONS iterations are enqueued at once -- as one hipGraph, built once -- with everything the host
 * would decide in between (how many parents, where the survivors go, the incumbent, whether to stop) decided by
 * single-workgroup kernels from state in device memory; the host reads the totals once per burst. */

static int enqueue_burst(csgpu_search *s, hipStream_t st) {
  const int n = s->n;
  const int64_t bound = s->parents_max * s->max_width; /* children of one iteration at most */
  const long long room_limit = pool_room_limit(s);
  const uint64_t *d_children = (const uint64_t *)(s->d_counters + C_TOTAL_CHILDREN);
  const int sense = objective_sense(s->objective);
  const int cpb = scatter_cpb(n, bound);
  const int split = s->path == PATH_BURST_SPLIT;
  const unsigned burst_wgs = (unsigned)((s->parents_max + BURST_PPW - 1) / BURST_PPW); /* <= BURST_WGS_MAX: plan_path */
  /* Without expression-tree clauses a complete consistent child IS a solution, and evaluating the root (eval_wand over
   * every clause, eval.c:233-255) can only say "true": every clause is a binary relation or a two-literal disjunction
   * whose revision on valued operands fails exactly when it is violated, and each was revised after the last of its
   * variables became a value (in this node or in the ancestor that valued it; the root's own valued clauses by the root
   * phase).  The launch that would say so is left out (CSGPU_SEARCH_EVAL=1 keeps it: tests compare the two). */
  const int *truth = s->burst_no_eval ? (const int *)NULL : (const int *)s->d_truth;
  for (int it = 0; it < BURST_ITERATIONS; it++) {
    if (split) {
      hipLaunchKernelGGL(cs_burst_branch, dim3(burst_wgs), dim3(1024), 0, st, s->pool, n, s->d_counters, s->d_burst,
                         s->objective, (long long)s->max_width, (long long)s->cap, room_limit, s->holes, s->d_choice,
                         s->d_block_sum, s->d_block_skip, (const cs_val *)s->d_child_states,
                         (const int *)s->d_complete_list, truth, s->obj_var, s->d_solutions,
                         (long long)s->max_solutions, s->d_best_solution, s->d_best, s->d_stream, (long long)s->stream_cap);
      hipLaunchKernelGGL(cs_burst_emit, dim3(burst_wgs), dim3(1024), 0, st, s->d_nodes, s->d_counters, s->d_burst,
                         s->objective, (const cs_choice *)s->d_choice, (const int *)s->d_block_sum,
                         (const int *)s->d_block_skip);
    } else
      hipLaunchKernelGGL(cs_expand_burst, dim3(1), dim3(1024), 0, st, s->pool, n, s->d_nodes, s->d_counters, s->d_burst,
                         s->objective, (long long)s->max_width, (long long)s->cap, room_limit, s->holes,
                         (const cs_val *)s->d_child_states, (const int *)s->d_complete_list, truth,
                         s->obj_var, s->d_solutions, (long long)s->max_solutions, s->d_best_solution, s->d_best,
                         s->d_stream, (long long)s->stream_cap);
    if (s->fw > 0)
      TRY(csgpu_internal_propagate_fb(s->m, (const csgpu_val *)s->pool, (const uint64_t *)s->pool_forb, s->d_nodes,
                                      (csgpu_val *)s->d_child_states, (uint64_t *)s->d_child_forb, s->d_results, bound,
                                      d_children, st));
    else
      TRY(csgpu_internal_propagate_objdev(s->m, (const csgpu_val *)s->pool, s->d_nodes, (csgpu_val *)s->d_child_states,
                                          s->d_results, bound, d_children, CS_DOM_MIN, CS_DOM_MAX,
                                          sense ? (const int32_t *)s->d_best : NULL, sense, st));
    if (s->prefer_failing)
      hipLaunchKernelGGL(cs_prio_update, dim3((unsigned)((bound + SB - 1) / SB)), dim3(SB), 0, st, (const csgpu_result *)s->d_results,
                         (const csgpu_node *)s->d_nodes, (int)bound, (const unsigned long long *)d_children, n, s->fail_var_known,
                         s->d_prio);
    if (split) {
      hipLaunchKernelGGL(cs_burst_count, dim3(BURST_CLASS_WGS), dim3(1024), 0, st, (const csgpu_result *)s->d_results,
                         (const unsigned long long *)s->d_counters, s->d_block_surv, s->d_block_comp, s->d_block_cuts,
                         s->d_block_props, s->d_block_revs);
      hipLaunchKernelGGL(cs_burst_assign, dim3(BURST_CLASS_WGS), dim3(1024), 0, st, (const csgpu_result *)s->d_results,
                         s->d_dest, s->d_complete_list, s->d_counters, s->d_burst, (const int *)s->d_block_surv,
                         (const int *)s->d_block_comp, (const int *)s->d_block_cuts, (const int *)s->d_block_props,
                         (const int *)s->d_block_revs, (const cs_val *)s->d_child_states, s->pool, n,
                         (const unsigned long long *)s->d_child_forb, s->pool_forb, s->fw);
    } else {
      hipLaunchKernelGGL(cs_classify_small, dim3(1), dim3(1024), 0, st, s->d_results, s->d_dest, s->d_complete_list,
                         s->d_counters, s->d_burst);
      hipLaunchKernelGGL(cs_scatter, dim3((unsigned)((bound + cpb - 1) / cpb)), dim3(SB), 0, st, s->d_child_states, s->d_dest,
                         s->d_counters, 0ll, n, s->pool, s->d_child_forb, s->pool_forb, s->fw, cpb,
                         (const unsigned long long *)(s->d_burst + B_SCATTER_BASE));
    }
    if (truth != NULL)
      TRY(csgpu_internal_eval_list(s->m, (const csgpu_val *)s->d_child_states, s->d_complete_list,
                                   (const uint64_t *)(s->d_counters + C_COMPLETE), bound, s->d_truth, st));
  }
  /* the last iteration's accept (the others ran at the head of the following expansion) */
  hipLaunchKernelGGL(cs_accept_burst, dim3(1), dim3(256), 0, st, s->d_child_states, s->d_complete_list, truth, n,
                     s->objective, s->obj_var, s->d_counters, s->d_burst, s->d_solutions, (long long)s->max_solutions,
                     s->d_best_solution, s->d_best, s->d_stream, (long long)s->stream_cap);
  HIP_OK(hipGetLastError());
  return CSGPU_OK;
}

/* up to `budget` iterations; *done = how many had parents */
static int run_burst(csgpu_search *s, int64_t budget, int64_t *done) {
  TRY(flush_accept_results(s));
  if (!s->sw.graph_off && (s->burst_exec == NULL || s->burst_limit != s->parents_max)) {
    drop_burst_graph(s);
    hipGraph_t graph = NULL;
    if (hipStreamBeginCapture(s->burst_stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
      const int rc = enqueue_burst(s, s->burst_stream);
      const hipError_t e = hipStreamEndCapture(s->burst_stream, &graph);
      if (rc != CSGPU_OK) {
        if (graph != NULL) (void)hipGraphDestroy(graph);
        return rc;
      }
      if (e == hipSuccess && graph != NULL && hipGraphInstantiate(&s->burst_exec, graph, NULL, NULL, 0) != hipSuccess)
        s->burst_exec = NULL;
      if (graph != NULL) (void)hipGraphDestroy(graph);
    }
    (void)hipGetLastError();
    s->burst_limit = s->parents_max;
  }
  unsigned long long *h = s->h_burst;
  memset(h, 0, sizeof(unsigned long long) * B_COUNT);
  h[B_TOP] = (unsigned long long)s->top;
  h[B_BUDGET] = (unsigned long long)(budget < BURST_ITERATIONS ? budget : BURST_ITERATIONS);
  h[B_LIMIT] = (unsigned long long)s->parents_limit;
  h[B_LIMIT_MAX] = (unsigned long long)s->parents_max;
  h[B_BACKLOG_DIV] = (unsigned long long)s->sw.backlog_div; /* a share of the pool per iteration, within [B_LIMIT, B_LIMIT_MAX] */
  h[B_ITER_BASE] = (unsigned long long)s->st.iterations;
  h[B_PEAK] = (unsigned long long)s->peak;
  HIP_OK(hipMemcpyAsync(s->d_burst, h, sizeof(unsigned long long) * B_COUNT, hipMemcpyHostToDevice, s->burst_stream));
  if (s->burst_exec != NULL)
    HIP_OK(hipGraphLaunch(s->burst_exec, s->burst_stream));
  else
    TRY(enqueue_burst(s, s->burst_stream));
  HIP_OK(hipMemcpyAsync(h, s->d_burst, sizeof(unsigned long long) * B_COUNT, hipMemcpyDeviceToHost, s->burst_stream));
  HIP_OK(hipMemcpyAsync(h + B_COUNT, s->d_counters, sizeof(unsigned long long) * C_COUNT, hipMemcpyDeviceToHost,
                        s->burst_stream));
  HIP_OK(hipMemcpyAsync(h + B_COUNT + C_COUNT, s->d_best, sizeof(int), hipMemcpyDeviceToHost, s->burst_stream));
  HIP_OK(hipStreamSynchronize(s->burst_stream));
  if (s->sw.trace)
    fprintf(stderr, "burst: iters %llu top %llu nodes %llu cuts %llu | surv %llu complete %llu children %llu solutions %llu stored %llu best %d\n",
            h[B_ITERS], h[B_TOP], h[B_NODES], h[B_CUTS], h[B_COUNT + C_SURVIVORS], h[B_COUNT + C_COMPLETE],
            h[B_COUNT + C_TOTAL_CHILDREN], h[B_COUNT + C_SOLUTIONS], h[B_COUNT + C_STORED], (int)(unsigned)h[B_COUNT + C_BEST]);
  if (h[B_ERROR] != 0ull) return fail(CSGPU_E_LIMIT, "state pool is full");
  *done = (int64_t)h[B_ITERS];
  s->top = (int64_t)h[B_TOP];
  s->peak = (int64_t)h[B_PEAK];
  s->st.iterations += h[B_ITERS];
  s->st.nodes += h[B_NODES];
  s->st.cuts += h[B_CUTS];
  s->st.props += h[B_PROPS];
  s->st.revisions += h[B_REVS];
  s->st.solutions = h[B_COUNT + C_SOLUTIONS];
  if (s->d_stream != NULL) s->stream_rows = (int64_t)h[B_COUNT + C_STREAM] - s->stream_head;
  if (s->objective == CS_OBJ_MIN || s->objective == CS_OBJ_MAX) s->st.best = *(const int *)(h + B_COUNT + C_COUNT);
  if (h[B_IMPROVED] != 0ull) {
    s->have_best_solution = 1;
    s->best_solution_value = (int32_t)(uint32_t)h[B_IMPROVED];
  }
  return CSGPU_OK;
}

/* a restart: the pool emptied and the seeds put back, without being recorded as new seeds */
static int restart_from_seeds(csgpu_search *s) {
  s->st.restarts++;
  s->top = 0;
  const int keep_flag = s->restart_on_improvement;
  const int64_t keep = s->restart_base;
  s->restart_on_improvement = 0;
  s->restart_base = 0;
  const int rc = csgpu_search_put(s, (const csgpu_val *)s->seed, s->seed_count);
  s->restart_base = keep;
  s->restart_on_improvement = keep_flag;
  return rc;
}

extern "C" int csgpu_search_run(csgpu_search *s, int64_t max_iterations, csgpu_search_stats *stats) {
  if (s == NULL || stats == NULL) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  if (s->stream_failed) return fail(CSGPU_E_STATE, "the solution stream overflowed: reset the engine");
  for (int64_t it = 0; it < max_iterations; it++) {
    if (s->top == 0) break;
    if (s->objective == CS_OBJ_ANY && s->st.solutions > 0) break;
    /* the solution stream: stop (not done) while it cannot take the worst case of the next iteration -- ALL: every
     * child of one parent; otherwise one row per iteration, so a burst takes at most as many iterations as there are
     * free rows.  The caller drains and runs on. */
    if (s->d_stream != NULL && stream_room(s) < (s->objective == CS_OBJ_ALL ? s->max_width : 1)) break;
    int64_t steps = 1; /* iterations this pass of the loop made */
    const int32_t best_before = s->st.best;
    const int restarts_on = s->restart_base > 0 && s->seed_count > 0 && s->st.solutions == 0;
    if (burst_path(s)) {
      int64_t budget = max_iterations - it;
      if (s->d_stream != NULL && budget > stream_room(s)) budget = stream_room(s);
      if (restarts_on) { /* stop where check_restart would fire */
        const int64_t until = (int64_t)s->luby_threshold * s->restart_base + 1 - s->since_restart;
        if (until < budget) budget = until < 1 ? 1 : until;
      }
      TRY(run_burst(s, budget, &steps));
      if (steps == 0) break; /* nothing left to expand (or ANY solved) */
      it += steps - 1;
    } else {
      TRY(one_iteration(s));
    }
    /* a better solution restarts a MIN / MAX search from its seeds with the new bound (update_solution +
     * is_solution_restartable, csolve.c:216-219, 418-425) */
    if (s->restart_on_improvement && s->seed_count > 0 && s->top > 0) {
      TRY(flush_accept_results(s));
      if (s->st.best != best_before) TRY(restart_from_seeds(s));
    }
    /* check_restart (csolve.c:264-276) with Knuth's Luby sequence (csolve.c:76-83) */
    if (restarts_on && s->st.solutions == 0 &&
        (s->since_restart += steps) > (int64_t)s->luby_threshold * s->restart_base) {
      s->since_restart = 0;
      cs_luby_next(&s->luby_threshold, &s->luby_counter);
      TRY(restart_from_seeds(s));
    }
  }
  TRY(flush_accept_results(s));
  if (s->d_stream != NULL) { /* the kernels' own test: a row that found no room is never dropped silently */
    unsigned long long err = 0ull;
    HIP_OK(hipMemcpy(&err, s->d_counters + C_STREAM_ERR, sizeof err, hipMemcpyDeviceToHost));
    if (err != 0ull) {
      s->stream_failed = 1; /* the host's count of rows may include rows that were not written */
      return fail(CSGPU_E_LIMIT, "solution stream overflow");
    }
  }
  s->st.pool = s->top;
  s->st.pool_peak = s->peak;
  s->st.done = s->top == 0 || (s->objective == CS_OBJ_ANY && s->st.solutions > 0);
  *stats = s->st;
  return CSGPU_OK;
}

extern "C" int64_t csgpu_search_solutions(const csgpu_search *s, int32_t *values, int64_t max) {
  if (s == NULL || values == NULL || max < 0) return CSGPU_E_ARG;
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  unsigned long long stored = 0;
  if (hipMemcpy(&stored, s->d_counters + C_STORED, sizeof stored, hipMemcpyDeviceToHost) != hipSuccess) return CSGPU_E_HIP;
  int64_t k = (int64_t)stored;
  if (k > s->max_solutions) k = s->max_solutions;
  if (k > max) k = max;
  if (k > 0 && hipMemcpy(values, s->d_solutions, (size_t)k * s->n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return CSGPU_E_HIP;
  return k;
}

extern "C" int csgpu_search_best_solution(const csgpu_search *s, int32_t *values) {
  if (s == NULL || values == NULL) return CSGPU_E_ARG;
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  /* with a shared incumbent another engine may hold the row that attains it */
  if (!s->have_best_solution || s->best_solution_value != s->st.best) return 0;
  if (hipMemcpy(values, s->d_best_solution, (size_t)s->n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return CSGPU_E_HIP;
  return 1;
}

/* ---- the solution stream: rows move out oldest first, from the ring's head; nothing else moves ---- */
static int stream_drain(csgpu_search *s, int32_t *values, int64_t max, int64_t *count, hipMemcpyKind kind, hipStream_t st) {
  if (s == NULL || values == NULL || count == NULL || max < 0) return fail(CSGPU_E_ARG, "bad argument");
  if (hipSetDevice(s->device) != hipSuccess) return fail(CSGPU_E_HIP, "hipSetDevice");
  if (s->d_stream == NULL) return fail(CSGPU_E_STATE, "no solution stream");
  if (s->stream_failed) return fail(CSGPU_E_STATE, "the solution stream overflowed: reset the engine");
  TRY(flush_accept_results(s)); /* the last iteration's accept: its rows (MIN / MAX: its pick) */
  *count = 0;
  const int64_t k = max < s->stream_rows ? max : s->stream_rows;
  if (k == 0) return CSGPU_OK;
  HIP_OK(hipDeviceSynchronize()); /* the engine's kernels run on the null stream and its burst stream */
  const size_t row = (size_t)s->n * sizeof(int32_t);
  /* at most two pieces: from the head to the ring's end, then from row 0 */
  const int64_t first = s->stream_head % s->stream_cap, part = k < s->stream_cap - first ? k : s->stream_cap - first;
  HIP_OK(hipMemcpyAsync(values, s->d_stream + (size_t)first * s->n, (size_t)part * row, kind, st));
  if (k > part) HIP_OK(hipMemcpyAsync(values + (size_t)part * s->n, s->d_stream, (size_t)(k - part) * row, kind, st));
  HIP_OK(hipStreamSynchronize(st));
  s->stream_head += k;
  s->stream_rows -= k;
  const unsigned long long head = (unsigned long long)s->stream_head; /* the freed rows may be written again */
  HIP_OK(hipMemcpy(s->d_counters + C_STREAM_HEAD, &head, sizeof head, hipMemcpyHostToDevice));
  *count = k;
  return CSGPU_OK;
}

extern "C" int csgpu_search_drain_solutions(csgpu_search *s, int32_t *values, int64_t max, int64_t *count) {
  return stream_drain(s, values, max, count, hipMemcpyDeviceToHost, (hipStream_t)0);
}

extern "C" int csgpu_search_drain_solutions_device(csgpu_search *s, int32_t *d_values, int64_t max, int64_t *count,
                                                   void *stream) {
  return stream_drain(s, d_values, max, count, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

extern "C" int csgpu_search_pending_solutions(const csgpu_search *s, int64_t *rows, int64_t *room) {
  if (s == NULL || rows == NULL || room == NULL) return fail(CSGPU_E_ARG, "bad argument");
  if (s->d_stream == NULL) return fail(CSGPU_E_STATE, "no solution stream");
  if (s->stream_failed) return fail(CSGPU_E_STATE, "the solution stream overflowed: reset the engine");
  *rows = s->stream_rows;
  *room = s->stream_cap - s->stream_rows;
  return CSGPU_OK;
}
