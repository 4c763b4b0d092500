/* cs_shard.c -- the sharded search of one node in host C: one engine per rank (process), coordinated through a region
 * of shared memory (include/csolve_gpu.h, csgpu_shard_*).  A restatement of ShardedSearch.run (csolve_amd/parallel.py)
 * with two differences:
 *   seeding   rank 0 alone expands the root and deals its frontier out through the inboxes (rank r keeps every
 *             world-th state starting at r), so the seeding counters are counted once and nothing is compared;
 *   transport a donor takes its states to the host, into the receiver's inbox; barrier; the receiver puts them (which
 *             rebuilds their forbidden sets); barrier.
 * The analogue of the reference's forked workers and the page they share (csolve.c:86-152, 190-244): the status words
 * are read between bursts of iterations without waiting for anyone, so an incumbent bounds the other ranks, a dry
 * rank's request for work, a timeout or an ANY solution are seen within one burst; the ranks meet only at exchanges.
 */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "cs_internal.h"

#define SHARD_MAGIC 0x3164726168735343ull /* "CSshard1" */
#define OBJ_ANY 0
#define OBJ_ALL 1
#define OBJ_MIN 2
#define OBJ_MAX 3

/* the words of one rank, each written by that rank alone (int64, a 256-byte row per rank) */
enum {
  W_WANT = 0,    /* the exchange (epoch) the rank waits at */
  W_BEST = 1,    /* its incumbent */
  W_FOUND = 2,   /* it has accepted a solution */
  W_POOL = 3,    /* its open states */
  W_TIMEOUT = 4, /* its clock ran out */
  W_TABLE = 8,   /* the exchange table, two by the parity of the epoch: pool, best, found, expired */
  W_FINAL = 16,  /* final counters: nodes, cuts, props, revisions, solutions, iterations, restarts, pool */
  W_FINAL_BEST = 24,
  W_HAS_BEST = 25, /* MIN / MAX: its engine holds a row attaining the node's optimum */
  W_INBOX = 26,    /* states waiting in its inbox */
  W_SEED = 27,     /* rank 0: the size of the frontier it deals out */
  WORDS = 32
};

typedef struct shard_header {
  uint64_t magic;
  int32_t world, n_vars;
  int64_t inbox_rows;
  int64_t reported; /* rows handed to the callbacks (under the lock) */
  pthread_mutex_t lock;
  pthread_barrier_t barrier;
} shard_header;

#define HEADER_BYTES ((sizeof(shard_header) + 255) / 256 * 256)

static int64_t *rank_words(void *region, int r) { return (int64_t *)((char *)region + HEADER_BYTES) + (size_t)r * WORDS; }

static csgpu_val *inbox(void *region, int r) {
  const shard_header *h = (const shard_header *)region;
  char *base = (char *)region + HEADER_BYTES + (size_t)h->world * WORDS * sizeof(int64_t);
  return (csgpu_val *)(base + (size_t)r * (size_t)h->inbox_rows * (size_t)h->n_vars * sizeof(csgpu_val));
}

static int64_t load(const int64_t *w) { return __atomic_load_n(w, __ATOMIC_ACQUIRE); }
static void store(int64_t *w, int64_t v) { __atomic_store_n(w, v, __ATOMIC_RELEASE); }

static int fail(int code, const char *msg) { return csgpu_internal_set_error(code, msg); }

#define TRY(expr)                                                              \
  do {                                                                         \
    const int rc_ = (expr);                                                    \
    if (rc_ != CSGPU_OK) return rc_;                                           \
  } while (0)

/* ---- the plan (parallel.plan_transfers) ---------------------------------------------------------------------- */

int csgpu_plan_transfers(const int64_t *pools, int world, int64_t low_water, int64_t max_give, int64_t *plan,
                         int *count) {
  if (pools == NULL || plan == NULL || count == NULL || world < 1 || world > 1024 || max_give < 1)
    return fail(CSGPU_E_ARG, "bad argument");
  int64_t p[1024];
  int order[1024];
  for (int r = 0; r < world; r++) {
    if (pools[r] < 0) return fail(CSGPU_E_ARG, "negative pool size");
    p[r] = pools[r];
    order[r] = r;
  }
  /* ascending by (pool, rank): an insertion sort, world is small */
  for (int i = 1; i < world; i++) {
    const int r = order[i];
    int j = i - 1;
    while (j >= 0 && (p[order[j]] > p[r] || (p[order[j]] == p[r] && order[j] > r))) {
      order[j + 1] = order[j];
      j--;
    }
    order[j + 1] = r;
  }
  int k = 0;
  for (int lo = 0, hi = world - 1; lo < hi; lo++, hi--) {
    const int poor = order[lo], rich = order[hi];
    if (p[poor] >= low_water) break;
    int64_t give = (p[rich] - p[poor]) / 2;
    if (give > max_give) give = max_give;
    if (give <= 0) break;
    plan[3 * k] = rich;
    plan[3 * k + 1] = poor;
    plan[3 * k + 2] = give;
    k++;
    p[rich] -= give;
    p[poor] += give;
  }
  *count = k;
  return CSGPU_OK;
}

/* ---- the region ------------------------------------------------------------------------------------------------ */

int csgpu_shard_region_size(int world, int n_vars, int64_t inbox_rows, size_t *bytes) {
  if (bytes == NULL || world < 1 || world > CSGPU_SHARD_MAX_WORLD || n_vars < 1 || inbox_rows < 1)
    return fail(CSGPU_E_ARG, "bad argument");
  const uint64_t row = (uint64_t)n_vars * sizeof(csgpu_val);
  if ((uint64_t)inbox_rows > ((uint64_t)1 << 40) / row) return fail(CSGPU_E_ARG, "inbox too large");
  *bytes = HEADER_BYTES + (size_t)world * WORDS * sizeof(int64_t) + (size_t)world * (size_t)inbox_rows * (size_t)row;
  return CSGPU_OK;
}

int csgpu_shard_region_init(void *region, size_t bytes, int world, int n_vars, int64_t inbox_rows) {
  size_t need = 0;
  TRY(csgpu_shard_region_size(world, n_vars, inbox_rows, &need));
  if (region == NULL || bytes < need) return fail(CSGPU_E_ARG, "region too small");
  memset(region, 0, HEADER_BYTES + (size_t)world * WORDS * sizeof(int64_t));
  shard_header *h = (shard_header *)region;
  h->world = world;
  h->n_vars = n_vars;
  h->inbox_rows = inbox_rows;
  pthread_mutexattr_t ma;
  pthread_barrierattr_t ba;
  if (pthread_mutexattr_init(&ma) != 0 || pthread_mutexattr_setpshared(&ma, PTHREAD_PROCESS_SHARED) != 0 ||
      pthread_mutex_init(&h->lock, &ma) != 0)
    return fail(CSGPU_E_STATE, "cannot create the region's lock");
  pthread_mutexattr_destroy(&ma);
  if (pthread_barrierattr_init(&ba) != 0 || pthread_barrierattr_setpshared(&ba, PTHREAD_PROCESS_SHARED) != 0 ||
      pthread_barrier_init(&h->barrier, &ba, (unsigned)world) != 0)
    return fail(CSGPU_E_STATE, "cannot create the region's barrier");
  pthread_barrierattr_destroy(&ba);
  __atomic_store_n(&h->magic, SHARD_MAGIC, __ATOMIC_RELEASE);
  return CSGPU_OK;
}

static int region_ok(void *region) {
  return region != NULL && __atomic_load_n(&((shard_header *)region)->magic, __ATOMIC_ACQUIRE) == SHARD_MAGIC;
}

int csgpu_shard_barrier(void *region) {
  if (!region_ok(region)) return fail(CSGPU_E_ARG, "not an initialised region");
  const int rc = pthread_barrier_wait(&((shard_header *)region)->barrier);
  if (rc != 0 && rc != PTHREAD_BARRIER_SERIAL_THREAD) return fail(CSGPU_E_STATE, "region barrier failed");
  return CSGPU_OK;
}

int csgpu_text_num_vars(const char *text, int weights_on, int *n_vars) {
  if (text == NULL || n_vars == NULL) return fail(CSGPU_E_ARG, "null argument");
  char err[256];
  cs_model *host = cs_model_parse(text, weights_on, err, sizeof err);
  if (host == NULL) return fail(CSGPU_E_PARSE, err);
  *n_vars = host->n_vars;
  cs_model_free(host);
  return CSGPU_OK;
}

void csgpu_shard_default_options(csgpu_shard_options *o) {
  if (o == NULL) return;
  memset(o, 0, sizeof *o);
  o->slice_iterations = 64;
  o->poll_iterations = 4;
  o->seed_states_per_rank = 64;
  o->low_water = 64;
}

/* ---- one rank ---------------------------------------------------------------------------------------------------- */

typedef struct shard {
  csgpu_search *s;
  void *region;
  shard_header *h;
  int rank, world, n, objective, obj_var;
  csgpu_shard_options o;
  int64_t *mine;
  int stream;            /* the engine's solution stream is on: drained after every run */
  int32_t *drained;      /* [stream rows][n] */
  int64_t drained_rows;
  int32_t *row;          /* [n] */
  double deadline;       /* monotonic seconds, 0 = none */
  int timed_out;
  csgpu_search_stats st;
} shard;

static double now(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static int expired(const shard *x) { return x->deadline > 0.0 && now() >= x->deadline; }

static int lock(shard *x) {
  return pthread_mutex_lock(&x->h->lock) == 0 ? CSGPU_OK : fail(CSGPU_E_STATE, "region lock failed");
}
static void unlock(shard *x) { pthread_mutex_unlock(&x->h->lock); }

/* the rows a run call left in the stream: ALL hands every one over, ANY its row if it is the node's first */
static int report_stream(shard *x) {
  if (!x->stream) return CSGPU_OK;
  for (;;) {
    int64_t got = 0;
    TRY(csgpu_search_drain_solutions(x->s, x->drained, x->drained_rows, &got));
    if (got == 0) return CSGPU_OK;
    if (x->objective == OBJ_ALL) {
      TRY(lock(x));
      x->h->reported += got;
      if (x->o.on_solution != NULL) x->o.on_solution(x->o.user, x->rank, x->drained, got, 0);
      unlock(x);
    }
    /* ANY: the same row as csgpu_search_solutions gives (report_any); MIN / MAX: the row is picked at the end */
  }
}

static int report_any(shard *x) {
  if (x->objective != OBJ_ANY || x->st.solutions == 0 || load(&x->mine[W_FOUND]) == 2) return CSGPU_OK;
  const int64_t k = csgpu_search_solutions(x->s, x->row, 1);
  if (k < 0) return (int)k;
  store(&x->mine[W_FOUND], 2); /* this rank's row has been offered */
  if (k == 0) return CSGPU_OK;
  TRY(lock(x));
  if (x->h->reported == 0) { /* the reference's found_any under its semaphore, csolve.c:207-244 */
    x->h->reported = 1;
    if (x->o.on_solution != NULL) x->o.on_solution(x->o.user, x->rank, x->row, 1, 0);
  }
  unlock(x);
  return CSGPU_OK;
}

static int run(shard *x, int64_t iterations) {
  TRY(csgpu_search_run(x->s, iterations, &x->st));
  TRY(report_stream(x));
  return report_any(x);
}

static void publish(shard *x, int64_t want) {
  int64_t *w = x->mine;
  store(&w[W_BEST], x->st.best);
  if (load(&w[W_FOUND]) == 0 && x->st.solutions > 0) store(&w[W_FOUND], 1);
  store(&w[W_POOL], x->st.pool);
  if (want >= 0) store(&w[W_WANT], want); /* last: the other words are in place when a neighbour sees the request */
}

static int64_t page_best(shard *x) {
  int64_t b = load(&rank_words(x->region, 0)[W_BEST]);
  for (int r = 1; r < x->world; r++) {
    const int64_t v = load(&rank_words(x->region, r)[W_BEST]);
    if (x->objective == OBJ_MIN ? v < b : v > b) b = v;
  }
  return b;
}

/* the neighbours' words: somebody waits at a later exchange, timed out, or (ANY) found a solution */
static int page_calls(shard *x, int64_t epoch) {
  for (int r = 0; r < x->world; r++) {
    const int64_t *w = rank_words(x->region, r);
    if (load(&w[W_WANT]) > epoch || load(&w[W_TIMEOUT]) != 0) return 1;
    if (x->objective == OBJ_ANY && load(&w[W_FOUND]) != 0) return 1;
  }
  return 0;
}

/* bursts of iterations until the slice is used up, the pool is dry, or the region calls the next exchange */
static int slice(shard *x, int64_t epoch) {
  int64_t burst = x->o.slice_iterations;
  if (x->world > 1) burst = x->o.poll_iterations;
  else if (x->deadline > 0.0) burst = x->o.poll_iterations > 16 ? x->o.poll_iterations : 16; /* only the clock */
  for (int64_t used = 0; used < x->o.slice_iterations;) {
    const int64_t k = burst < x->o.slice_iterations - used ? burst : x->o.slice_iterations - used;
    TRY(run(x, k));
    used += k;
    if (x->st.done || x->st.pool == 0) break;
    if (x->objective == OBJ_ANY && x->st.solutions > 0) break;
    if (expired(x)) {
      if (x->world > 1) store(&x->mine[W_TIMEOUT], 1);
      break;
    }
    if (x->world > 1) {
      publish(x, -1);
      if (x->objective == OBJ_MIN || x->objective == OBJ_MAX) TRY(csgpu_search_set_best(x->s, (int32_t)page_best(x)));
      if (page_calls(x, epoch)) break;
    }
  }
  return CSGPU_OK;
}

/* rank 0 expands the root and deals the frontier out: rank r keeps states r, r + world, ... (in chunks of an inbox) */
static int seed(shard *x, const csgpu_val *root) {
  const int world = x->world, n = x->n;
  const int64_t rows = x->h->inbox_rows;
  csgpu_val *frontier = NULL, *own = NULL;
  int rc = CSGPU_OK;
  if (x->rank == 0) {
    TRY(csgpu_search_put_host(x->s, root, 1));
    const int64_t want = x->o.seed_states_per_rank * world;
    TRY(run(x, 1));
    while (!x->st.done && x->st.pool < want) TRY(run(x, 1));
    int64_t k = x->st.pool;
    if (k > 0) {
      frontier = (csgpu_val *)malloc((size_t)k * n * sizeof(csgpu_val));
      own = (csgpu_val *)malloc((size_t)((k + world - 1) / world) * n * sizeof(csgpu_val));
      if (frontier == NULL || own == NULL) rc = fail(CSGPU_E_ARG, "out of memory");
      if (rc == CSGPU_OK) rc = csgpu_search_take_host(x->s, frontier, k, &k);
      int64_t j = 0;
      for (int64_t i = 0; rc == CSGPU_OK && i < k; i += world, j++)
        memcpy(own + (size_t)j * n, frontier + (size_t)i * n, (size_t)n * sizeof(csgpu_val));
      if (rc == CSGPU_OK) rc = csgpu_search_put_host(x->s, own, j);
      if (rc == CSGPU_OK) rc = csgpu_search_run(x->s, 0, &x->st);
    }
    store(&x->mine[W_SEED], rc == CSGPU_OK ? k : 0);
  }
  if (rc == CSGPU_OK) rc = csgpu_shard_barrier(x->region);
  const int64_t k = load(&rank_words(x->region, 0)[W_SEED]);
  const int64_t most = (k + world - 1) / world; /* rank 0's share, the largest */
  for (int64_t c = 0; rc == CSGPU_OK && c < most; c += rows) {
    if (x->rank == 0) {
      for (int r = 1; r < world; r++) {
        int64_t m = 0;
        for (int64_t i = (c * world) + r; i < k && m < rows; i += world, m++)
          memcpy(inbox(x->region, r) + (size_t)m * n, frontier + (size_t)i * n, (size_t)n * sizeof(csgpu_val));
        store(&rank_words(x->region, r)[W_INBOX], m);
      }
    }
    rc = csgpu_shard_barrier(x->region);
    if (rc == CSGPU_OK && x->rank != 0)
      rc = csgpu_search_put_host(x->s, inbox(x->region, x->rank), load(&x->mine[W_INBOX]));
    if (rc == CSGPU_OK) rc = csgpu_shard_barrier(x->region);
  }
  free(frontier);
  free(own);
  return rc;
}

/* incumbent, termination and work stealing at exchange `epoch`; *over = the search ends here on every rank */
static int exchange(shard *x, int64_t epoch, int *over) {
  const int world = x->world, parity = (int)(epoch & 1);
  int64_t *t = x->mine + W_TABLE + 4 * parity;
  store(&t[0], x->st.pool);
  store(&t[1], x->st.best);
  store(&t[2], x->st.solutions > 0);
  store(&t[3], expired(x));
  TRY(csgpu_shard_barrier(x->region));
  int64_t pools[CSGPU_SHARD_MAX_WORLD], best = 0, sum = 0;
  int found = 0;
  for (int r = 0; r < world; r++) {
    const int64_t *w = rank_words(x->region, r) + W_TABLE + 4 * parity;
    pools[r] = load(&w[0]);
    sum += pools[r];
    const int64_t b = load(&w[1]);
    if (r == 0 || (x->objective == OBJ_MIN ? b < best : b > best)) best = b;
    found |= load(&w[2]) != 0;
    if (load(&w[3]) != 0) x->timed_out = 1; /* one rank's clock is everybody's */
  }
  if (x->objective == OBJ_MIN || x->objective == OBJ_MAX) TRY(csgpu_search_set_best(x->s, (int32_t)best));
  *over = (x->objective == OBJ_ANY && found) || sum == 0 || x->timed_out;
  if (*over) return CSGPU_OK;
  int64_t plan[3 * (CSGPU_SHARD_MAX_WORLD / 2)];
  int moves = 0;
  TRY(csgpu_plan_transfers(pools, world, x->o.low_water, x->h->inbox_rows, plan, &moves));
  if (moves == 0) return CSGPU_OK;
  int receive = 0;
  for (int i = 0; i < moves; i++) {
    const int src = (int)plan[3 * i], dst = (int)plan[3 * i + 1];
    if (x->rank == src) {
      int64_t got = 0;
      TRY(csgpu_search_take_host(x->s, inbox(x->region, dst), plan[3 * i + 2], &got));
      store(&rank_words(x->region, dst)[W_INBOX], got);
    }
    receive |= x->rank == dst;
  }
  TRY(csgpu_shard_barrier(x->region));
  if (receive) TRY(csgpu_search_put_host(x->s, inbox(x->region, x->rank), load(&x->mine[W_INBOX])));
  return csgpu_shard_barrier(x->region); /* the inboxes are free again */
}

/* the counters of every rank summed, the node's best, and (MIN / MAX) the one row that attains it */
static int finish(shard *x, csgpu_search_stats *totals) {
  int64_t *f = x->mine + W_FINAL;
  const uint64_t mine[7] = {x->st.nodes, x->st.cuts, x->st.props, x->st.revisions, x->st.solutions,
                            x->st.iterations, x->st.restarts};
  for (int i = 0; i < 7; i++) store(&f[i], (int64_t)mine[i]);
  store(&f[7], x->st.pool);
  store(&x->mine[W_FINAL_BEST], x->st.best);
  if (x->world > 1) TRY(csgpu_shard_barrier(x->region));
  csgpu_search_stats T = x->st;
  uint64_t sums[7] = {0, 0, 0, 0, 0, 0, 0};
  int64_t pool = 0, best = 0;
  for (int r = 0; r < x->world; r++) {
    const int64_t *w = rank_words(x->region, r);
    for (int i = 0; i < 7; i++) sums[i] += (uint64_t)load(&w[W_FINAL + i]);
    pool += load(&w[W_FINAL + 7]);
    const int64_t b = load(&w[W_FINAL_BEST]);
    if (r == 0 || (x->objective == OBJ_MIN ? b < best : b > best)) best = b;
  }
  T.nodes = sums[0], T.cuts = sums[1], T.props = sums[2], T.revisions = sums[3];
  T.iterations = sums[5], T.restarts = sums[6];
  T.solutions = x->objective == OBJ_ANY ? (sums[4] > 0 ? 1 : 0) : sums[4];
  T.pool = pool;
  if (x->objective == OBJ_MIN || x->objective == OBJ_MAX) T.best = (int32_t)best;
  T.done = pool == 0 || (x->objective == OBJ_ANY && T.solutions > 0);
  if ((x->objective == OBJ_MIN || x->objective == OBJ_MAX) && T.solutions > 0) {
    TRY(csgpu_search_set_best(x->s, T.best));
    const int has = csgpu_search_best_solution(x->s, x->row);
    if (has < 0) return has;
    store(&x->mine[W_HAS_BEST], has == 1);
    if (x->world > 1) TRY(csgpu_shard_barrier(x->region));
    int first = -1;
    for (int r = 0; r < x->world && first < 0; r++)
      if (load(&rank_words(x->region, r)[W_HAS_BEST]) != 0) first = r;
    if (first == x->rank) {
      TRY(lock(x));
      x->h->reported = 1;
      if (x->o.on_solution != NULL)
        x->o.on_solution(x->o.user, x->rank, x->row, 1, x->obj_var >= 0 ? x->row[x->obj_var] : T.best);
      unlock(x);
    }
  }
  if (x->world > 1) TRY(csgpu_shard_barrier(x->region)); /* every row is out before anyone goes on */
  *totals = T;
  return CSGPU_OK;
}

int csgpu_shard_run(csgpu_search *s, void *region, int rank, const csgpu_val *root, const csgpu_shard_options *options,
                    csgpu_search_stats *local, csgpu_search_stats *totals) {
  if (s == NULL || options == NULL || local == NULL || totals == NULL) return fail(CSGPU_E_ARG, "bad argument");
  if (!region_ok(region)) return fail(CSGPU_E_ARG, "not an initialised region");
  shard x;
  memset(&x, 0, sizeof x);
  x.s = s;
  x.region = region;
  x.h = (shard_header *)region;
  x.rank = rank;
  x.world = x.h->world;
  x.o = *options;
  int restarts = 0;
  int64_t stream_rows = 0;
  if (csgpu_internal_search_info(s, &x.objective, &x.obj_var, &x.n, &restarts, &stream_rows) != CSGPU_OK)
    return fail(CSGPU_E_ARG, "bad argument");
  if (rank < 0 || rank >= x.world || x.n != x.h->n_vars) return fail(CSGPU_E_ARG, "rank or n_vars does not fit the region");
  if (rank == 0 && root == NULL) return fail(CSGPU_E_ARG, "rank 0 needs the root state");
  if (x.o.slice_iterations < 1 || x.o.poll_iterations < 1 || x.o.seed_states_per_rank < 1 || x.o.low_water < 0 ||
      x.o.time_limit < 0.0)
    return fail(CSGPU_E_ARG, "bad shard options");
  if (x.world > 1 && restarts)
    return fail(CSGPU_E_STATE, "restarts re-put only the states put before the first iteration: turn them off on every rank");
  x.stream = stream_rows > 0;
  if (x.objective == OBJ_ALL && x.o.on_solution != NULL && !x.stream)
    return fail(CSGPU_E_STATE, "ALL reports its rows through the solution stream: turn it on");
  x.mine = rank_words(region, rank);
  x.drained_rows = stream_rows;
  x.drained = (int32_t *)malloc((size_t)(x.drained_rows > 0 ? x.drained_rows : 1) * (size_t)x.n * sizeof(int32_t));
  x.row = (int32_t *)malloc((size_t)x.n * sizeof(int32_t));
  if (x.drained == NULL || x.row == NULL) {
    free(x.drained);
    free(x.row);
    return fail(CSGPU_E_ARG, "out of memory");
  }
  if (x.o.time_limit > 0.0) x.deadline = now() + x.o.time_limit;

  int rc = CSGPU_OK;
  if (x.world == 1) {
    rc = csgpu_search_put_host(s, root, 1);
    if (rc == CSGPU_OK) rc = csgpu_search_run(s, 0, &x.st);
    while (rc == CSGPU_OK) {
      rc = slice(&x, 0);
      if (rc != CSGPU_OK || x.st.done) break;
      if (expired(&x)) {
        x.timed_out = 1;
        break;
      }
    }
  } else {
    /* every row is initialised before anyone reads a neighbour's */
    store(&x.mine[W_BEST], x.objective == OBJ_MIN ? INT32_MAX : (x.objective == OBJ_MAX ? INT32_MIN : 0));
    store(&x.mine[W_WANT], 0);
    rc = csgpu_shard_barrier(region);
    if (rc == CSGPU_OK) rc = seed(&x, root);
    if (rc == CSGPU_OK) rc = csgpu_search_run(s, 0, &x.st);
    for (int64_t epoch = 0; rc == CSGPU_OK;) {
      rc = slice(&x, epoch);
      if (rc != CSGPU_OK) break;
      epoch++;
      publish(&x, epoch);
      int over = 0;
      rc = exchange(&x, epoch, &over);
      if (rc != CSGPU_OK || over) break;
      rc = csgpu_search_run(s, 0, &x.st);
    }
  }
  if (rc == CSGPU_OK) rc = finish(&x, totals);
  if (rc == CSGPU_OK) *local = x.st;
  free(x.drained);
  free(x.row);
  return rc;
}
