/* cs_main.c -- command-line front for the GPU engine with the reference's input and output
 * conventions:
 *   input  : the csolve problem text (file argument, "-" or none = stdin), reference src/main.c:313-322
 *   output : "INFEASIBLE PROBLEM" (parser.y:70-72), one line per solution
 *            "#1: SOLUTION: X1 = 8, X2 = 2, ..., BEST: 0"  (print.c:24-31, 49-70, csolve.c:233-234),
 *            a final statistics line "#1: CALLS: n, CUTS: n, PROPS: n, CONFL: 0, RESTARTS: n, ...,
 *            SOLUTIONS: n" (csolve.c:54-58, csolve.h:469-479) and "NO SOLUTION FOUND" (csolve.c:184-186)
 *   errors : "<argv0>: error: <message>" on stderr, exit status 1 (print.c:73-94)
 * Options (reference src/main.c:51-130): -w <bool> weights; -o <order> none | smallest-domain | largest-domain |
 * smallest-value | largest-value (the engine's default is smallest-domain, the reference's none); -f <bool> prefer
 * failing variables; -r <int> restart frequency (ANY: Luby restarts every r x 64-parent iterations, 0 = none; MIN /
 * MAX: r > 0 also restarts on every better solution, csolve.c:418-425); -t <int> time limit in seconds (0 = none);
 * -c <bool> is accepted (this engine does not learn conflict clauses: the drop-in does); -s -b -p -m -M
 * size the reference's host structures and are accepted and ignored.
 * -j <int> workers (the reference's worker processes, csolve.c:105-152): absent, 0 or 1 = one engine in this process,
 * the path below.  N >= 2 = min(N, 8) ranks (8: one per GPU of a node, and well under the 16 processes a GPU may
 * have open), each a fresh process of this program started with posix_spawn, rank r on device r % devices, coordinated
 * in C by csgpu_shard_run (include/csolve_gpu.h) through a region of shared memory (a memfd the ranks inherit, which
 * also carries the problem text).  This launcher process only parses, spawns and supervises: it makes no HIP call, so no
 * process that has used the GPU is ever forked or exec'd.  A rank that fails makes the launcher end the others
 * (SIGTERM, SIGKILL after 5 s) and exit 1; ranks die with the launcher (PR_SET_PDEATHSIG).  The ranks run without
 * restarts (-r is accepted and not applied: a restart would drop the subtrees a rank was given).  Output: the
 * "#<r+1>: SOLUTION: ..." lines as the ranks report them (ALL every row, ANY the node's first, MIN / MAX the optimal
 * row at the end), written under the region's lock; then one statistics line per rank, "#2" ... "#N" and "#1" last,
 * each with its rank's CALLS / CUTS / PROPS and the node's SOLUTIONS; then "NO SOLUTION FOUND" if that is 0.
 * The search order differs from the reference's (batched expansion), so CALLS/CUTS and WHICH
 * solution an ANY run prints are engine-specific; the set of solutions and the optimum are not.
 * ALL prints every solution (csolve.c:222-244): the engine's solution stream is drained and printed after every
 * csgpu_search_run call, so the SOLUTION lines are as many as the final SOLUTIONS count, in the engine's order.
 */
#define _GNU_SOURCE
#include <errno.h>
#include <signal.h>
#include <spawn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include "../../include/csolve_gpu.h"

static const char *prog = "csolve_gpu";

static void die(const char *msg) {
  fprintf(stderr, "%s: error: %s\n", prog, msg);
  exit(EXIT_FAILURE);
}

static void print_solution(const csgpu_model *m, int n, const int32_t *vals, int32_t best, int worker) {
  printf("#%d: SOLUTION: ", worker);
  for (int v = 0; v < n; v++) printf("%s = %d, ", csgpu_model_var_name(m, v), vals[v]);
  printf("BEST: %d\n", best);
}

#define STREAM_BYTES (16 << 20) /* ALL: the solution stream (and the host buffer it is drained into), drained after every run call */

static char *read_all(FILE *f) {
  size_t cap = 1 << 16, n = 0;
  char *buf = (char *)malloc(cap);
  for (;;) {
    size_t got = fread(buf + n, 1, cap - n - 1, f);
    n += got;
    if (got == 0) break;
    if (n + 1 >= cap) buf = (char *)realloc(buf, cap *= 2);
  }
  buf[n] = '\0';
  return buf;
}

typedef struct options {
  int weights, order, prefer, have_strategy;
  long restart_freq, time_max, jobs;
  const char *path;
} options;

static void parse_options(int argc, char **argv, int first, options *o) {
  o->weights = 1, o->order = -1, o->prefer = 0, o->have_strategy = 0;
  o->restart_freq = -1, o->time_max = 0, o->jobs = 0;
  o->path = NULL;
  for (int i = first; i < argc; i++) {
    if (argv[i][0] == '-' && argv[i][1] != '\0') {
      if (strchr("bcfjmMoprstw", argv[i][1]) == NULL || i + 1 >= argc)
        die("usage: csolve_gpu [-w <bool>] [-o <order>] [-f <bool>] [-r <int>] [-t <seconds>] [-c <bool>] [-j <int>] [<file>]");
      const char *arg = argv[i + 1];
      switch (argv[i][1]) {
      case 'w': o->weights = strcmp(arg, "true") == 0; break;
      case 'f': o->prefer = strcmp(arg, "true") == 0; o->have_strategy = 1; break;
      case 'o':
        o->order = strcmp(arg, "none") == 0 ? 0 : strcmp(arg, "smallest-domain") == 0 ? 1 : strcmp(arg, "largest-domain") == 0 ? 2 :
                   strcmp(arg, "smallest-value") == 0 ? 3 : strcmp(arg, "largest-value") == 0 ? 4 : -2;
        if (o->order == -2) die("invalid order"); /* ERROR_MSG_INVALID_STRATEGY_ORDER */
        o->have_strategy = 1;
        break;
      case 'r': o->restart_freq = strtol(arg, NULL, 10); break;
      case 't': o->time_max = strtol(arg, NULL, 10); break;
      case 'j': o->jobs = strtol(arg, NULL, 10); break;
      default: break; /* -c -s -b -p -m -M: accepted */
      }
      i++;
    } else {
      o->path = argv[i];
    }
  }
}

/* ---- -j N: the launcher and its ranks ---------------------------------------------------------------------------- */

#define RANK_FLAG "--shard-rank" /* hidden: argv[0] --shard-rank <rank> <world> <memfd> <launcher pid> <the user's arguments> */
#define MAX_RANKS CSGPU_SHARD_MAX_WORLD
#define INBOX_BYTES (4 << 20) /* per rank: the states one transfer or one chunk of the seed frontier moves at most */

extern char **environ;

static size_t text_offset(size_t region_bytes) { return (region_bytes + 4095) / 4096 * 4096; }

static const csgpu_model *rank_model;

static void print_rows(void *user, int rank, const int32_t *rows, int64_t count, int32_t best) {
  (void)user;
  const int n = csgpu_model_num_vars(rank_model);
  for (int64_t i = 0; i < count; i++) print_solution(rank_model, n, rows + i * n, best, rank + 1);
  fflush(stdout); /* under the region's lock: the lines of two ranks never interleave */
}

static int run_rank(int argc, char **argv) {
  const int rank = atoi(argv[2]), world = atoi(argv[3]), fd = atoi(argv[4]);
  const pid_t launcher = (pid_t)atol(argv[5]);
  if (prctl(PR_SET_PDEATHSIG, SIGKILL) != 0 || getppid() != launcher) die("rank: the launcher is gone");
  options opt;
  parse_options(argc, argv, 6, &opt);
  struct stat sb;
  if (fstat(fd, &sb) != 0) die("rank: cannot read the shared region");
  char *base = (char *)mmap(NULL, (size_t)sb.st_size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  if (base == MAP_FAILED) die("rank: cannot map the shared region");
  close(fd);
  size_t region_bytes = 0;
  int64_t text_len = 0;
  memcpy(&region_bytes, base + (size_t)sb.st_size - sizeof region_bytes, sizeof region_bytes);
  memcpy(&text_len, base + text_offset(region_bytes), sizeof text_len);
  const char *text = base + text_offset(region_bytes) + sizeof text_len;

  const int devices = csgpu_device_count();
  if (devices < 0) die(csgpu_last_error());
  if (devices == 0) die("no HIP device");
  if (csgpu_set_device(rank % devices) != CSGPU_OK) die(csgpu_last_error());

  csgpu_model *m = NULL;
  if (csgpu_model_from_text(text, opt.weights, &m) != CSGPU_OK) die(csgpu_last_error());
  int32_t st = 0;
  if (csgpu_model_root_propagate(m, &st) != CSGPU_OK) die(csgpu_last_error());
  if (st >= 0) {
    if (csgpu_model_normalize(m) != CSGPU_OK || csgpu_model_root_propagate(m, &st) != CSGPU_OK) die(csgpu_last_error());
  }
  if (st < 0) { /* every rank finds the same: rank 0 says it */
    if (rank == 0) printf("INFEASIBLE PROBLEM\n");
    return EXIT_SUCCESS;
  }
  if (csgpu_model_finalize(m) != CSGPU_OK) die(csgpu_last_error());
  const int n = csgpu_model_num_vars(m);
  csgpu_search *s = NULL;
  if (csgpu_search_create(m, 1 << 21, 1 << 17, &s) != CSGPU_OK) die(csgpu_last_error());
  if (opt.have_strategy && csgpu_search_set_strategy(s, opt.order < 0 ? 1 : opt.order, opt.prefer) != CSGPU_OK)
    die(csgpu_last_error());
  /* -r is not applied: a restart re-puts the states put before the first iteration and drops the rank's later share */
  if (csgpu_search_set_restart(s, 0) != CSGPU_OK || csgpu_search_set_restart_on_improvement(s, 0) != CSGPU_OK)
    die(csgpu_last_error());
  if (csgpu_model_objective(m) == 1) {
    int64_t stream_rows = (int64_t)STREAM_BYTES / ((int64_t)n * (int64_t)sizeof(int32_t));
    if (stream_rows < 1024) stream_rows = 1024;
    if (csgpu_search_set_solution_stream(s, stream_rows) != CSGPU_OK) die(csgpu_last_error());
  }
  csgpu_val *root = NULL;
  if (rank == 0) {
    root = (csgpu_val *)malloc((size_t)n * sizeof *root);
    csgpu_model_get_domains(m, root);
  }
  csgpu_shard_options so;
  csgpu_shard_default_options(&so);
  so.time_limit = (double)opt.time_max;
  so.on_solution = print_rows;
  rank_model = m;
  csgpu_search_stats local, totals;
  if (csgpu_shard_run(s, base, rank, root, &so, &local, &totals) != CSGPU_OK) die(csgpu_last_error());
  /* one statistics line per rank, "#2" ... "#N", then "#1" */
  for (int turn = 1; turn <= world; turn++) {
    if (rank == turn % world) {
      printf("#%d: CALLS: %lu, CUTS: %lu, PROPS: %lu, CONFL: 0, RESTARTS: %lu, LEVEL: 0/%d, AVG LEVEL: 0.000000, MEM: 0, CMEM: 0, SOLUTIONS: %lu\n",
             rank + 1, (unsigned long)local.nodes, (unsigned long)local.cuts, (unsigned long)local.props,
             (unsigned long)local.restarts, n, (unsigned long)totals.solutions);
      if (rank == 0 && totals.solutions == 0) printf("NO SOLUTION FOUND\n");
      fflush(stdout);
    }
    if (csgpu_shard_barrier(base) != CSGPU_OK) die(csgpu_last_error());
  }
  csgpu_search_free(s);
  csgpu_model_free(m);
  free(root);
  return EXIT_SUCCESS;
}

static double seconds_now(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

/* SIGTERM to the ranks still running, SIGKILL to those left after 5 s; reaps them all */
static void end_ranks(pid_t *pids, int world, int *alive) {
  for (int r = 0; r < world; r++)
    if (pids[r] > 0) kill(pids[r], SIGTERM);
  const double until = seconds_now() + 5.0;
  int killed = 0;
  while (*alive > 0) {
    int status = 0;
    const pid_t p = waitpid(-1, &status, killed ? 0 : WNOHANG);
    if (p > 0) {
      for (int r = 0; r < world; r++)
        if (pids[r] == p) pids[r] = 0, (*alive)--;
    } else if (p < 0 && errno != EINTR) {
      break;
    } else if (p == 0 && seconds_now() >= until) {
      for (int r = 0; r < world; r++)
        if (pids[r] > 0) kill(pids[r], SIGKILL);
      killed = 1;
    } else if (p == 0) {
      const struct timespec nap = {0, 10 * 1000 * 1000};
      nanosleep(&nap, NULL);
    }
  }
}

/* the launcher: the region in a memfd, one fresh process per rank, supervision.  No HIP call in this process (the
 * problem text is parsed on the host only, to size the inboxes and to report a syntax error once). */
static int launch(int world, const options *opt, char *text, int argc, char **argv) {
  int n = 0;
  if (csgpu_text_num_vars(text, opt->weights, &n) != CSGPU_OK) die(csgpu_last_error());
  if (n < 1) die("the problem has no variables");
  int64_t inbox_rows = INBOX_BYTES / ((int64_t)n * (int64_t)sizeof(csgpu_val));
  if (inbox_rows < 64) inbox_rows = 64;
  size_t region_bytes = 0;
  if (csgpu_shard_region_size(world, n, inbox_rows, &region_bytes) != CSGPU_OK) die(csgpu_last_error());
  /* [region][pad][int64 text length][text][NUL]...[size_t region bytes] */
  const int64_t text_len = (int64_t)strlen(text);
  const size_t total = text_offset(region_bytes) + sizeof text_len + (size_t)text_len + 1 + sizeof region_bytes;
  const int fd = memfd_create("csolve_gpu_shard", 0); /* inherited by the ranks */
  if (fd < 0 || ftruncate(fd, (off_t)total) != 0) die("cannot create the shared region");
  char *base = (char *)mmap(NULL, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  if (base == MAP_FAILED) die("cannot map the shared region");
  if (csgpu_shard_region_init(base, region_bytes, world, n, inbox_rows) != CSGPU_OK) die(csgpu_last_error());
  memcpy(base + text_offset(region_bytes), &text_len, sizeof text_len);
  memcpy(base + text_offset(region_bytes) + sizeof text_len, text, (size_t)text_len + 1);
  memcpy(base + total - sizeof region_bytes, &region_bytes, sizeof region_bytes);
  free(text);

  char srank[16], sworld[16], sfd[16], sparent[24];
  snprintf(sworld, sizeof sworld, "%d", world);
  snprintf(sfd, sizeof sfd, "%d", fd);
  snprintf(sparent, sizeof sparent, "%ld", (long)getpid());
  char **cargv = (char **)calloc((size_t)argc + 6, sizeof *cargv);
  cargv[0] = argv[0];
  cargv[1] = (char *)RANK_FLAG;
  cargv[2] = srank;
  cargv[3] = sworld;
  cargv[4] = sfd;
  cargv[5] = sparent;
  for (int i = 1; i < argc; i++) cargv[5 + i] = argv[i];
  fflush(NULL);
  pid_t pids[MAX_RANKS] = {0};
  int alive = 0;
  for (int r = 0; r < world; r++) {
    snprintf(srank, sizeof srank, "%d", r);
    const int e = posix_spawn(&pids[r], "/proc/self/exe", NULL, NULL, cargv, environ);
    if (e != 0) {
      pids[r] = 0;
      fprintf(stderr, "%s: error: cannot start rank %d: %s\n", prog, r, strerror(e));
      end_ranks(pids, world, &alive);
      return EXIT_FAILURE;
    }
    alive++;
  }
  int failed = 0;
  while (alive > 0) {
    int status = 0;
    const pid_t p = waitpid(-1, &status, 0);
    if (p < 0) {
      if (errno == EINTR) continue;
      break;
    }
    int r = -1;
    for (int i = 0; i < world; i++)
      if (pids[i] == p) r = i;
    if (r < 0) continue;
    pids[r] = 0;
    alive--;
    if (WIFEXITED(status) && WEXITSTATUS(status) == 0) continue;
    if (WIFSIGNALED(status))
      fprintf(stderr, "%s: error: rank %d died of signal %d\n", prog, r, WTERMSIG(status));
    else
      fprintf(stderr, "%s: error: rank %d exited with status %d\n", prog, r, WEXITSTATUS(status));
    failed = 1;
    end_ranks(pids, world, &alive); /* a rank is never started again */
  }
  free(cargv);
  munmap(base, total);
  close(fd);
  return failed ? EXIT_FAILURE : EXIT_SUCCESS;
}

int main(int argc, char **argv) {
  prog = argv[0];
  if (argc >= 6 && strcmp(argv[1], RANK_FLAG) == 0) return run_rank(argc, argv);
  options opt;
  parse_options(argc, argv, 1, &opt);
  const int weights = opt.weights, order = opt.order, prefer = opt.prefer, have_strategy = opt.have_strategy;
  const long restart_freq = opt.restart_freq, time_max = opt.time_max;
  const char *path = opt.path;
  FILE *in = stdin;
  if (path != NULL && strcmp(path, "-") != 0 && (in = fopen(path, "r")) == NULL) die("cannot open input");
  char *text = read_all(in);
  if (opt.jobs >= 2) return launch(opt.jobs < MAX_RANKS ? (int)opt.jobs : MAX_RANKS, &opt, text, argc, argv);

  csgpu_model *m = NULL;
  if (csgpu_model_from_text(text, weights, &m) != CSGPU_OK) die(csgpu_last_error());
  free(text);
  int32_t st = 0;
  if (csgpu_model_root_propagate(m, &st) != CSGPU_OK) die(csgpu_last_error());
  if (st >= 0) {
    if (csgpu_model_normalize(m) != CSGPU_OK || csgpu_model_root_propagate(m, &st) != CSGPU_OK) die(csgpu_last_error());
  }
  if (st < 0) {
    printf("INFEASIBLE PROBLEM\n");
    return EXIT_SUCCESS;
  }
  if (csgpu_model_finalize(m) != CSGPU_OK) die(csgpu_last_error());

  const int n = csgpu_model_num_vars(m);
  csgpu_search *s = NULL;
  if (csgpu_search_create(m, 1 << 21, 1 << 17, &s) != CSGPU_OK) die(csgpu_last_error());
  csgpu_val *root = (csgpu_val *)malloc((size_t)n * sizeof *root);
  csgpu_model_get_domains(m, root);
  if (have_strategy && csgpu_search_set_strategy(s, order < 0 ? 1 : order, prefer) != CSGPU_OK) die(csgpu_last_error());
  if (restart_freq >= 0) {
    if (csgpu_search_set_restart(s, restart_freq) != CSGPU_OK) die(csgpu_last_error());
    if (csgpu_search_set_restart_on_improvement(s, restart_freq > 0) != CSGPU_OK) die(csgpu_last_error());
  }
  const int obj = csgpu_model_objective(m), ov = csgpu_model_objective_var(m);
  const int all = obj == 1;
  int32_t *drained = NULL;
  /* rows of the stream: 16 MiB of them, and at least one parent's children (the engine refuses fewer) */
  int64_t stream_rows = (int64_t)STREAM_BYTES / ((int64_t)n * (int64_t)sizeof(int32_t));
  if (stream_rows < 1024) stream_rows = 1024;
  if (all) {
    if (csgpu_search_set_solution_stream(s, stream_rows) != CSGPU_OK) die(csgpu_last_error());
    drained = (int32_t *)malloc((size_t)stream_rows * (size_t)n * sizeof(int32_t));
    if (drained == NULL) die("out of memory");
  }
  if (csgpu_search_put_host(s, root, 1) != CSGPU_OK) die(csgpu_last_error());
  csgpu_search_stats stats;
  /* -t: the clock is looked at between slices of 64 iterations (the reference's SIGALRM sets a flag its loop tests).
   * ALL: a run call also returns when the stream is full; what it holds is printed before the next one. */
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (;;) {
    if (csgpu_search_run(s, time_max > 0 ? 64 : (int64_t)1 << 60, &stats) != CSGPU_OK) die(csgpu_last_error());
    if (all) {
      int64_t got = 0;
      if (csgpu_search_drain_solutions(s, drained, stream_rows, &got) != CSGPU_OK) die(csgpu_last_error());
      for (int64_t i = 0; i < got; i++) print_solution(m, n, drained + i * n, 0, 1);
    }
    if (stats.done) break;
    if (time_max > 0) {
      clock_gettime(CLOCK_MONOTONIC, &t1);
      if ((double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec) >= (double)time_max) break;
    }
  }

  int32_t *vals = (int32_t *)malloc((size_t)n * sizeof(int32_t));
  if (!all) {
    int64_t k = csgpu_search_solutions(s, vals, 1);
    if (obj >= 2) /* MIN/MAX: the solution that attains the optimum (the reference's last line) */
      k = csgpu_search_best_solution(s, vals) == 1 ? 1 : 0;
    if (k == 1) print_solution(m, n, vals, (obj >= 2 && ov >= 0) ? vals[ov] : 0, 1);
  }
  printf("#1: CALLS: %lu, CUTS: %lu, PROPS: %lu, CONFL: 0, RESTARTS: %lu, LEVEL: 0/%d, AVG LEVEL: 0.000000, MEM: 0, CMEM: 0, SOLUTIONS: %lu\n",
         (unsigned long)stats.nodes, (unsigned long)stats.cuts, (unsigned long)stats.props,
         (unsigned long)stats.restarts, n, (unsigned long)stats.solutions);
  if (stats.solutions == 0) printf("NO SOLUTION FOUND\n");
  csgpu_search_free(s);
  csgpu_model_free(m);
  free(root); free(vals); free(drained);
  return EXIT_SUCCESS;
}
