/* cs_capi.hip -- implementation of the C ABI declared in include/csolve_gpu.h.
 * Host orchestration only: parsing / indexing / table building happen in the C files
 * next to this one, every interval computation happens in the kernels of
 * cs_kernels.hip.h.  Nothing here evaluates or narrows a domain on the CPU. */
#include <hip/hip_runtime.h>
#include <chrono>

#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "../../include/csolve_gpu.h"
#include "cs_kernels.hip.h"
#include "cs_shave.hip.h"
#include "cs_step.hip.h"
#include "cs_dive.hip.h"
#include "cs_walk.hip.h"
#include "cs_chain.hip.h"
#include "cs_internal.h"

static thread_local char g_err[512] = "";

static int set_err(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

/* shared with cs_search.hip */
extern "C" int csgpu_internal_set_error(int code, const char *msg) { return set_err(code, "%s", msg); }

#define HIP_TRY(expr)                                                          \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess)                                                      \
      return set_err(CSGPU_E_HIP, "%s: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

#define CS_TICKET_SLOTS 1024
#define CS_TICKET_STREAMS 64
#define CS_TICKET_SLOT_WORDS (CS_SHAVE_SHARDS * CS_SHAVE_TICKET_STRIDE)

#define CS_CU_LDS (160u * 1024u) /* LDS of one CU */

/* one kernel a model may launch, resolved by csgpu_model_finalize (fn == NULL: the model does not qualify) */
struct cs_planned {
  const void *fn; /* the instantiation; its LDS attribute was set for `lds` */
  size_t lds;     /* dynamic LDS bytes per workgroup */
  int waves;      /* waves per workgroup */
  int per_cu;     /* resident workgroups per CU */
};

/* the kernels of the csgpu_solve_many family (cs_dive.hip.h): one loop, compiled five times, and the four that branch on
 * the allowed values (planned only for root domains of at most CS_DIVE_ALLOWED_WIDTH values) */
enum { MANY_PLAIN, MANY_CK, MANY_UPTO, MANY_RESTART, MANY_STREAM, MANY_ALLOWED, MANY_ALLOWED_UPTO, MANY_ALLOWED_CK,
       MANY_ALLOWED_UPTO_CK, MANY_FAMILIES };
static const char *const many_kernel_name[MANY_FAMILIES] = { "cs_dive_shave", "cs_dive_resume", "cs_dive_upto", "cs_dive_restart",
                                                             "cs_dive_stream", "cs_dive_allowed", "cs_dive_allowed_upto",
                                                             "cs_dive_allowed_resume", "cs_dive_allowed_upto_resume" };
#define MANY_BY_ALLOWED(family) ((family) >= MANY_ALLOWED && (family) <= MANY_ALLOWED_UPTO_CK)
#define CS_DIVE_ALLOWED_WIDTH 128 /* the widest root domain the allowed sets of cs_dive_allowed hold (four 32-bit words) */

/* the kernels of the csgpu_solve_many_clauses family (cs_walk.hip.h): one loop on kernel 6's fixpoint, compiled nine times
 * with the records in registers (WALK_FAMILIES of them, planned together for at most 512 clauses) and twice with the
 * records in LDS (WALK_WIDE, WALK_WIDE_CK: csgpu_solve_many_clauses_wide, planned for themselves) */
enum { WALK_PLAIN, WALK_CK, WALK_UPTO, WALK_RESTART, WALK_STREAM, WALK_FROM, WALK_ORDER, WALK_ORDER_CK, WALK_ORDER_FROM,
       WALK_FAMILIES, WALK_WIDE = WALK_FAMILIES, WALK_WIDE_CK, WALK_SLOTS };
static const char *const walk_kernel_name[WALK_SLOTS] = { "cs_walk_clauses", "cs_walk_resume", "cs_walk_upto", "cs_walk_restart",
                                                          "cs_walk_stream", "cs_walk_from", "cs_walk_order",
                                                          "cs_walk_order_resume", "cs_walk_order_from", "cs_walk_wide",
                                                          "cs_walk_wide_resume" };

/* every kernel of the batched fixpoint, its tracing variants, the search steps and the server, for one model */
struct cs_kernel_plan {
  cs_planned events, traced;       /* kernel 1; its tracing variant (one node) */
  cs_planned rounds;               /* kernel 6 */
  int rounds_cpl;                  /* its clauses per lane (1, 2, 4, 8) */
  cs_planned lds;                  /* kernel 2 */
  cs_planned bitset;               /* kernel 3 */
  cs_planned regs[4];              /* kernel 4: [fast | sets_only << 1] */
  cs_planned packed;               /* kernel 5 */
  int packed_nodes;                /* its nodes per wave */
  cs_planned shave, shave_trace;   /* kernel 7 (the instantiation whose FULL matches the model); its tracing variant */
  cs_planned server;               /* the resident single-node server */
  cs_planned step_shave, step_packed, step_import;
  cs_planned dive[MANY_FAMILIES];  /* by MANY_*: the first five all or none, the four MANY_ALLOWED* with them unless the
                                      domains are too wide; not among csgpu_internal_plan_symbol's families */
  cs_planned walk[WALK_SLOTS];     /* by WALK_*: kernel 6's instantiation of each of the first WALK_FAMILIES, all or none;
                                      WALK_WIDE and WALK_WIDE_CK, both or neither; no plan families either */
  int full;                        /* the variables fill the lanes of a wave (64, 128 or 256 of them) */
  int step_kind;                   /* csgpu_internal_step_kind */
  int max_width;                   /* widest root interval, at least 2 */
};

struct csgpu_model {
  cs_model *host;
  int from_dump;     /* clause lists came with the file: keep them */
  int not_root;      /* host domains are not the root state: no entailed-clause elimination */
  int finalized;
  cs_dev_image *img; /* search image */
  /* device copies of the image */
  int *d_adj_off, *d_adj, *d_clause, *d_tree_off, *d_tnode, *d_tkid, *d_tree_want, *d_lit, *d_clause_by_kind;
  cs_tables tab;
  size_t slice;      /* LDS bytes per node instance (16-byte aligned) */
  int has_tree_adj;  /* some adjacency entry is a tree clause */
  int packed_bias;   /* kernel 5: largest root_lo - dense_dmin */
  int packed_nw;     /* kernel 5: set words per variable it works on (1: all root domains within 32 values) */
  int kernel_choice; /* 0 auto, 1 general, 2 LDS-resident, 3 forbidden sets, 4 forbidden sets in registers, 5 = 4 with
                        several nodes per wave */
  cs_kernel_plan plan;
  void *d_adj_packed;
  int lds_adj_global; /* kernel 2 reads its adjacency through L2 (the lists would leave LDS for fewer than 16 waves) */
  int k2_csz;         /* kernel 2's nodes per chunk when CSGPU_K2_CSZ sets them (0: by the batch) */
  int shave_static;   /* CSGPU_SHAVE_STATIC: kernel 7 without tickets */
  int step_chunk_max; /* cs_step_packed: most parents per ticket */
  size_t k1_tab_bytes; /* general kernel: adj_off + adj + lit copied into LDS by every workgroup (0: read through L2) */
  int fb_words;      /* forbidden-set words per variable (0 = not eligible) */
  size_t dense_bytes; /* the dense pair table of kernels 4, 5 and 7 */
  void *d_dense_tab;
  void *d_packed_tab; /* kernel 5: 16-bit table relative to the pushing variable */
  int *d_root_lo;
  int *d_root_hi;    /* csgpu_solve_many: a root row must lie inside the root domains */
  /* csgpu_solve_many: the waves' stacks (sized at the first call, grown when a later call needs more bytes: more waves,
   * or the n + 1 frames per wave of cs_walk_restart after a call with n) and the ticket counters of cs_dive_shave, which
   * the kernel leaves at zero */
  void *d_many_stack;
  size_t many_stack_bytes;
  unsigned *d_many_tickets;
  cs_val *d_walk_root; /* csgpu_solve_many_clauses: the root domains, which a root row must lie inside */
  int *d_sym_off;
  void *d_sym_packed;
  int n_cus;
  /* kernel 7: ticket counters of its work distribution (cs_shave.hip.h).  One slot (CS_SHAVE_SHARDS counters on
   * their own 64-byte lines) per stream that launches it -- launches of one stream are ordered, and the kernel
   * leaves its counters at zero -- and one slot of its own for every launch that is being captured into a
   * hipGraph (graphs captured on one stream may be replayed on different ones at the same time). */
  unsigned *d_tickets;
  int ticket_slots, ticket_streams, ticket_reserved;
  void *ticket_stream[CS_TICKET_STREAMS];
  /* staging of csgpu_propagate_one */
  /* pinned host memory mapped into the device's address space: the kernel reads the state and the node record
   * from it and writes the result and the new state back, no staging copies */
  unsigned char *h_one;          /* [state | node | result | state_out] */
  /* csgpu_propagate_one_traced: clause of every adjacency entry (device), the log and its counter (mapped host
   * memory), allocated at the first traced call */
  int *d_adj_clause;
  int32_t *h_trace;
  unsigned *h_trace_n;
  int trace_cap;
  cs_val *d_one_in, *d_one_out;  /* device views of the four parts */
  cs_node_in *d_one_node;
  cs_node_out *d_one_res;
  int engines; /* csgpu_search objects built on this model (they hold pointers into its device tables) */
  /* csgpu_propagate_one_chain (cs_chain.hip.h): clause shapes and lists on the device, the frame stack, the mapped
   * host buffers; chain_state: 0 not built yet, 1 ready, -1 the model does not qualify */
  int chain_state;
  cs_chain_clause *d_chain_cl;
  int *d_chain_off, *d_chain_list;
  cs_chain_frame *d_chain_frames;
  int *h_chain_out; /* mapped: [4] out, then the bumps */
  /* the resident single-node server (cs_shave_server): its mailbox in coherent host memory, its stream, the last
   * request number; srv_off: not used for this model (it does not qualify, or CSGPU_SERVER=0) */
  unsigned char *h_box;   /* [cs_mailbox_head | state_in | state_out | trace] */
  size_t box_state_off, box_out_off, box_trace_off;
  hipStream_t srv_stream;
  unsigned srv_seq;
  int srv_off, srv_launched;
  double srv_seconds[4]; /* host copy in, ring + wait, copy out, (re)starts -- csgpu_debug_one_timing */
  uint64_t srv_calls, srv_starts;
  /* staging of csgpu_propagate_values (mapped pinned memory, grown on demand) */
  unsigned char *h_values, *d_values;
  size_t values_cap;
};

extern "C" const char *csgpu_last_error(void) { return g_err; }

/* Wait for the null stream by polling.  The single-node entries (the drop-in's calls) are a launch of a few
 * microseconds followed by a wait: hipStreamSynchronize in a process that has not asked for spinning blocks in the
 * kernel driver and is woken 50-100 us later (the reference's driver linked on this library measured 75 us per call
 * where a python loop, whose runtime spins, measured 19 us for the same calls). */
static int wait_null_stream(void) {
  for (;;) {
    const hipError_t e = hipStreamQuery(NULL);
    if (e == hipSuccess) return CSGPU_OK;
    if (e != hipErrorNotReady) return set_err(CSGPU_E_HIP, "hipStreamQuery: %s", hipGetErrorString(e));
  }
}

extern "C" int csgpu_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return set_err(CSGPU_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

extern "C" int csgpu_set_device(int device) {
  HIP_TRY(hipSetDevice(device));
  return CSGPU_OK;
}

/* ---- helpers of the search driver (cs_arith.h), exported so that the reference's unit vectors run against the
 * very functions the kernels, the engine and the drop-in use ---------------------------------------------------- */

static int objective_sense(int objective) { return objective == CS_OBJ_MIN ? 1 : (objective == CS_OBJ_MAX ? 2 : 0); }

extern "C" int csgpu_objective_better(int objective, csgpu_val value, int32_t best) {
  return cs_objective_better(objective_sense(objective), cs_interval(value.lo, value.hi), best);
}
extern "C" csgpu_val csgpu_objective_bound(int objective, csgpu_val value, int32_t best) {
  const cs_val v = cs_objective_bound(objective_sense(objective), cs_interval(value.lo, value.hi), best);
  csgpu_val out;
  out.lo = v.lo;
  out.hi = v.hi;
  return out;
}
extern "C" int32_t csgpu_objective_best(int objective, csgpu_val value, int32_t best) {
  return cs_objective_best(objective_sense(objective), cs_interval(value.lo, value.hi), best);
}
extern "C" void csgpu_luby_next(uint64_t *threshold, uint64_t *counter) {
  if (threshold != NULL && counter != NULL) cs_luby_next(threshold, counter);
}
extern "C" int csgpu_step_check(csgpu_val bounds, uint32_t iter) {
  return cs_step_check(cs_interval(bounds.lo, bounds.hi), iter);
}
extern "C" uint64_t csgpu_branch_key(int order, int prefer_failing, csgpu_val value, int64_t prio, int32_t index) {
  return cs_branch_key_of(order, prefer_failing, cs_interval(value.lo, value.hi), prio, index);
}
extern "C" int32_t csgpu_step_val(csgpu_val bounds, uint32_t iter, uint32_t seed) {
  return cs_step_val(cs_interval(bounds.lo, bounds.hi), iter, seed);
}
extern "C" int32_t csgpu_many_value(uint32_t seed, uint32_t run, int32_t var, csgpu_val bounds, uint32_t j, int32_t flags) {
  return cs_many_value(seed, run, var, cs_interval(bounds.lo, bounds.hi), j, flags);
}

/* ---- host model ------------------------------------------------------------------ */

static int wrap_model(cs_model *host, int from_dump, csgpu_model **out) {
  csgpu_model *m = (csgpu_model *)calloc(1, sizeof *m);
  if (m == NULL) { cs_model_free(host); return set_err(CSGPU_E_ARG, "out of memory"); }
  m->host = host;
  m->from_dump = from_dump;
  *out = m;
  return CSGPU_OK;
}

extern "C" int csgpu_model_from_text(const char *text, int weights_on, csgpu_model **out) {
  if (text == NULL || out == NULL) return set_err(CSGPU_E_ARG, "null argument");
  char err[256];
  cs_model *host = cs_model_parse(text, weights_on, err, sizeof err);
  if (host == NULL) return set_err(CSGPU_E_PARSE, "%s", err);
  return wrap_model(host, 0, out);
}

extern "C" int csgpu_model_from_file(const char *path, int weights_on, csgpu_model **out) {
  if (path == NULL || out == NULL) return set_err(CSGPU_E_ARG, "null argument");
  FILE *f = fopen(path, "rb");
  if (f == NULL) return set_err(CSGPU_E_ARG, "%s: cannot open", path);
  fseek(f, 0, SEEK_END);
  long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  char *text = (char *)malloc((size_t)len + 1);
  size_t got = fread(text, 1, (size_t)len, f);
  fclose(f);
  text[got] = '\0';
  int rc = csgpu_model_from_text(text, weights_on, out);
  free(text);
  return rc;
}

extern "C" int csgpu_model_from_dump(const char *path, csgpu_model **out) {
  if (path == NULL || out == NULL) return set_err(CSGPU_E_ARG, "null argument");
  char err[256];
  cs_model *host = cs_model_load(path, err, sizeof err);
  if (host == NULL) return set_err(CSGPU_E_ARG, "%s", err);
  if (host->clause_node == NULL) {
    cs_model_free(host);
    return set_err(CSGPU_E_ARG, "%s: model file has no clause index", path);
  }
  return wrap_model(host, 1, out);
}

/* internal (cs_internal.h): wrap a host model built by other host code of this package
 * (the drop-in shim); takes ownership.  lists_final: keep the clause index it carries. */
extern "C" int csgpu_model_from_host(cs_model *host, int lists_final, int domains_are_root, csgpu_model **out) {
  if (host == NULL || out == NULL) return set_err(CSGPU_E_ARG, "null argument");
  int rc = wrap_model(host, lists_final, out);
  if (rc == CSGPU_OK) (*out)->not_root = !domains_are_root;
  return rc;
}

extern "C" cs_model *csgpu_model_host(csgpu_model *m) { return m ? m->host : NULL; }

static void server_stop(csgpu_model *m);
static void server_reap(csgpu_model *m);
/* Models whose resident server may be running.  hipFree, hipDeviceSynchronize and friends wait for EVERY stream of the
 * device, the server's included -- they would sit out its idle time-out (2 ms) each.  Entry points that allocate, free
 * or synchronise device-wide therefore ask the servers of this process to leave first (a flag in the mailbox: the wave
 * is gone within microseconds); the next single-node call starts one again. */
static csgpu_model *g_srv_models[16];
static void quiesce_servers(void) {
  for (int i = 0; i < 16; i++)
    if (g_srv_models[i] != NULL) server_stop(g_srv_models[i]);
}

static void free_device(csgpu_model *m) {
  (void)hipFree(m->d_chain_cl); (void)hipFree(m->d_chain_off); (void)hipFree(m->d_chain_list); (void)hipFree(m->d_chain_frames);
  if (m->h_chain_out != NULL) (void)hipHostFree(m->h_chain_out);
  m->d_chain_cl = NULL; m->d_chain_off = NULL; m->d_chain_list = NULL; m->d_chain_frames = NULL; m->h_chain_out = NULL;
  m->chain_state = 0;
  quiesce_servers(); /* before anything is freed: this model's resident wave reads the tables, and hipFree waits for all of them */
  for (int i = 0; i < 16; i++)
    if (g_srv_models[i] == m) g_srv_models[i] = NULL;
  if (m->h_box != NULL) (void)hipHostFree(m->h_box);
  m->h_box = NULL;
  if (m->srv_stream != NULL) (void)hipStreamDestroy(m->srv_stream);
  m->srv_stream = NULL;
  m->srv_off = 0;
  (void)hipFree(m->d_adj_off); (void)hipFree(m->d_adj); (void)hipFree(m->d_clause); (void)hipFree(m->d_clause_by_kind);
  (void)hipFree(m->d_tree_off); (void)hipFree(m->d_tnode); (void)hipFree(m->d_tkid); (void)hipFree(m->d_tree_want);
  (void)hipFree(m->d_lit);
  m->d_tree_want = NULL;
  m->d_lit = NULL;
  (void)hipFree(m->d_adj_packed);
  (void)hipFree(m->d_root_lo);
  (void)hipFree(m->d_root_hi);
  (void)hipFree(m->d_many_stack);
  (void)hipFree(m->d_many_tickets);
  (void)hipFree(m->d_walk_root);
  m->d_walk_root = NULL;
  m->d_root_hi = NULL;
  m->d_many_stack = NULL;
  m->d_many_tickets = NULL;
  m->many_stack_bytes = 0;
  (void)hipFree(m->d_sym_off);
  (void)hipFree(m->d_sym_packed);
  (void)hipFree(m->d_dense_tab);
  (void)hipFree(m->d_packed_tab);
  m->d_packed_tab = NULL;
  (void)hipFree(m->d_tickets);
  m->d_tickets = NULL;
  m->ticket_slots = m->ticket_streams = m->ticket_reserved = 0;
  m->d_sym_off = NULL;
  m->d_sym_packed = NULL;
  m->d_dense_tab = NULL;
  m->d_adj_packed = NULL;
  m->d_root_lo = NULL;
  memset(&m->plan, 0, sizeof m->plan);
  m->fb_words = 0;
  (void)hipHostFree(m->h_one);
  m->h_one = NULL;
  (void)hipFree(m->d_adj_clause);
  m->d_adj_clause = NULL;
  if (m->h_trace != NULL) (void)hipHostFree(m->h_trace);
  m->h_trace = NULL;
  m->h_trace_n = NULL;
  m->trace_cap = 0;
  if (m->h_values != NULL) (void)hipHostFree(m->h_values);
  m->h_values = m->d_values = NULL;
  m->values_cap = 0;
  m->d_adj_off = m->d_adj = m->d_clause = m->d_tree_off = m->d_tnode = m->d_tkid = m->d_clause_by_kind = NULL;
  m->d_one_in = m->d_one_out = NULL;
  m->d_one_node = NULL;
  m->d_one_res = NULL;
  cs_dev_image_free(m->img);
  m->img = NULL;
}

extern "C" void csgpu_model_free(csgpu_model *m) {
  if (m == NULL) return;
  free_device(m);
  cs_model_free(m->host);
  free(m);
}

extern "C" int csgpu_model_num_vars(const csgpu_model *m) { return m ? m->host->n_vars : CSGPU_E_ARG; }
extern "C" int csgpu_model_num_clauses(const csgpu_model *m) {
  if (m == NULL) return CSGPU_E_ARG;
  /* the clause index is built on demand (it only depends on the trees and the domains) */
  if (m->host->clause_node == NULL && m->host->root >= 0 && cs_model_index(m->host) != 0) return CSGPU_E_ARG;
  return m->host->n_clauses;
}
extern "C" int csgpu_model_objective(const csgpu_model *m) { return m ? m->host->objective : CSGPU_E_ARG; }
extern "C" int csgpu_model_objective_var(const csgpu_model *m) { return m ? m->host->obj_var : CSGPU_E_ARG; }

extern "C" const char *csgpu_model_var_name(const csgpu_model *m, int var) {
  if (m == NULL || var < 0 || var >= m->host->n_vars) return NULL;
  return m->host->names[var];
}

extern "C" int csgpu_model_get_domains(const csgpu_model *m, csgpu_val *out) {
  if (m == NULL || out == NULL) return set_err(CSGPU_E_ARG, "null argument");
  memcpy(out, m->host->dom, (size_t)m->host->n_vars * sizeof(cs_val));
  return CSGPU_OK;
}

extern "C" int csgpu_model_set_domains(csgpu_model *m, const csgpu_val *in) {
  if (m == NULL || in == NULL) return set_err(CSGPU_E_ARG, "null argument");
  memcpy(m->host->dom, in, (size_t)m->host->n_vars * sizeof(cs_val));
  return CSGPU_OK;
}

extern "C" void csgpu_set_linear_fast_paths(int on) { cs_dev_linear_fast_paths = on != 0; }

extern "C" int csgpu_model_device_info(const csgpu_model *m, int64_t info[8]) {
  if (m == NULL || info == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (m->img == NULL) return set_err(CSGPU_E_STATE, "device tables are not built");
  info[0] = m->img->n_adj;
  info[1] = m->img->n_ne;
  info[2] = m->img->n_tree_clauses;
  info[3] = m->img->n_tnodes;
  info[4] = (int64_t)m->slice;
  info[5] = m->img->max_list;
  info[6] = m->img->n_skip;
  info[7] = m->img->max_tree;
  return CSGPU_OK;
}

/* ---- device image ------------------------------------------------------------------ */

struct dev_tables_owner {
  int *adj_off, *adj, *clause, *tree_off, *tnode, *tkid, *tree_want, *lit, *clause_by_kind;
};

static int upload(const void *src, size_t bytes, int **dst) {
  HIP_TRY(hipMalloc((void **)dst, bytes ? bytes : 16));
  if (bytes) HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return CSGPU_OK;
}

static int upload_image(const cs_dev_image *g, dev_tables_owner *o, cs_tables *t) {
  int rc;
  memset(o, 0, sizeof *o);
  if ((rc = upload(g->adj_off, ((size_t)g->n_vars + 1) * 4, &o->adj_off))) return rc;
  if ((rc = upload(g->adj, (size_t)(g->n_adj ? g->n_adj : 1) * 8, &o->adj))) return rc;
  if ((rc = upload(g->clause, (size_t)(g->n_clauses ? g->n_clauses : 1) * 16, &o->clause))) return rc;
  {
    /* the clause records once more, sorted by kind -- =, <, !=, then disjunctions, trees, constants -- for the
     * kernel that gives every lane its own clauses (kernel 6): a round revises ALL clauses whatever their order, and 64
     * lanes of one kind run one path instead of all of them one after the other */
    const int32_t nc = g->n_clauses;
    int32_t *sorted = (int32_t *)malloc((size_t)(nc ? nc : 1) * 16);
    if (sorted == NULL) return set_err(CSGPU_E_LIMIT, "out of memory");
    static const int order[] = { CS_CL_EQ, CS_CL_LT, CS_CL_NE, CS_CL_OR2, CS_CL_TREE, CS_CL_SKIP };
    int32_t k = 0;
    for (size_t q = 0; q < sizeof order / sizeof order[0]; q++)
      for (int32_t c = 0; c < nc; c++)
        if (g->clause[4 * c] == order[q]) { memcpy(sorted + 4 * k, g->clause + 4 * c, 16); k++; }
    rc = k == nc ? upload(sorted, (size_t)(nc ? nc : 1) * 16, &o->clause_by_kind) : set_err(CSGPU_E_STATE, "clause of unknown kind");
    free(sorted);
    if (rc) return rc;
  }
  if ((rc = upload(g->tree_off, ((size_t)g->n_trees + 1) * 4, &o->tree_off))) return rc;
  if ((rc = upload(g->tnode, (size_t)(g->n_tnodes ? g->n_tnodes : 1) * 16, &o->tnode))) return rc;
  if ((rc = upload(g->tkid, (size_t)(g->n_tkids ? g->n_tkids : 1) * 4, &o->tkid))) return rc;
  if ((rc = upload(g->tree_want, (size_t)(g->n_trees ? g->n_trees : 1) * 8, &o->tree_want))) return rc;
  if ((rc = upload(g->lit, (size_t)(g->n_lits ? g->n_lits : 1) * 16, &o->lit))) return rc;
  t->n_vars = g->n_vars;
  t->n_clauses = g->n_clauses;
  t->n_words = (g->n_vars + 31) / 32;
  t->adj_off = o->adj_off;
  t->adj = (const int2 *)o->adj;
  t->clause = (const int4 *)o->clause;
  t->clause_by_kind = (const int4 *)o->clause_by_kind;
  t->tree_off = o->tree_off;
  t->tnode = (const int4 *)o->tnode;
  t->tkid = o->tkid;
  t->tree_want = (const int2 *)o->tree_want;
  t->lit = (const int4 *)o->lit;
  t->n_lits = g->n_lits;
  t->obj_var = -1;
  t->obj_lo = CS_DOM_MIN;
  t->obj_hi = CS_DOM_MAX;
  t->obj_best_dev = NULL;
  t->obj_sense = 0;
  return CSGPU_OK;
}

static void free_tables(dev_tables_owner *o) {
  (void)hipFree(o->adj_off); (void)hipFree(o->adj); (void)hipFree(o->clause); (void)hipFree(o->clause_by_kind);
  (void)hipFree(o->tree_off); (void)hipFree(o->tnode); (void)hipFree(o->tkid); (void)hipFree(o->tree_want);
  (void)hipFree(o->lit);
}

static int lds_limit(size_t bytes, const void *func) {
  if (bytes > CS_CU_LDS) return set_err(CSGPU_E_LIMIT, "%zu bytes of LDS per workgroup exceed the 160 KiB of a CU", bytes);
  if (bytes > 48u * 1024u)
    HIP_TRY(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return CSGPU_OK;
}

/* ---- root phase -------------------------------------------------------------------- */

extern "C" int csgpu_model_root_propagate(csgpu_model *m, int32_t *status) {
  return csgpu_model_root_propagate_limit(m, -1, status, NULL);
}

extern "C" int csgpu_model_root_propagate_limit(csgpu_model *m, int64_t limit, int32_t *status, int32_t *rounds) {
  if (m == NULL || status == NULL) return set_err(CSGPU_E_ARG, "null argument");
  quiesce_servers();
  cs_model *h = m->host;
  if (h->root < 0) return set_err(CSGPU_E_STATE, "model has no root");
  if (!m->from_dump && cs_model_index(h) != 0) return set_err(CSGPU_E_ARG, "%s", h->err);
  char err[200];
  cs_dev_image *g = cs_dev_image_build(h, 0, NULL, err, sizeof err);
  if (g == NULL) return set_err(CSGPU_E_LIMIT, "%s", err);

  dev_tables_owner own;
  cs_tables tab;
  int rc = upload_image(g, &own, &tab);
  cs_val *d_in = NULL, *d_out = NULL;
  cs_node_out *d_res = NULL;
  int *d_conv = NULL, conv = 1;
  cs_node_out res;
  const size_t nbytes = (size_t)(h->n_vars ? h->n_vars : 1) * sizeof(cs_val);
  const size_t lds = (size_t)h->n_vars * sizeof(cs_val) + 4 * sizeof(unsigned);
  hipError_t e = hipSuccess;
  if (rc == CSGPU_OK) rc = lds_limit(lds, (const void *)cs_propagate_sweeps);
  if (rc == CSGPU_OK) {
    if ((e = hipMalloc((void **)&d_in, nbytes)) != hipSuccess || (e = hipMalloc((void **)&d_out, nbytes)) != hipSuccess ||
        (e = hipMalloc((void **)&d_res, sizeof res)) != hipSuccess || (e = hipMalloc((void **)&d_conv, sizeof(int))) != hipSuccess ||
        (e = hipMemcpy(d_in, h->dom, (size_t)h->n_vars * sizeof(cs_val), hipMemcpyHostToDevice)) != hipSuccess)
      rc = set_err(CSGPU_E_HIP, "root propagate setup: %s", hipGetErrorString(e));
  }
  if (rc == CSGPU_OK) {
    /* propagate(root, limit) stops after limit + 1 sweeps (propagate.c:479-483) */
    const int max_rounds = limit < 0 || limit >= 0x7ffffffe ? 0x7fffffff : (int)limit + 1;
    /* All clauses of a round in parallel first: a round never narrows more than a sweep of the reference, so a
     * fixpoint (or an inconsistency) reached within the limit is the reference's.  Only when the limit cuts the
     * iteration short do the states depend on the order: then the same number of sweeps is run again from the
     * start in the reference's own order, one clause after the other (propagate.c:379-392, 474-485). */
    hipLaunchKernelGGL(cs_propagate_sweeps, dim3(1), dim3(CS_BLOCK), lds, 0, tab, d_in, d_out, d_res, max_rounds, 0, d_conv);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess ||
        (e = hipMemcpy(&res, d_res, sizeof res, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(&conv, d_conv, sizeof conv, hipMemcpyDeviceToHost)) != hipSuccess)
      rc = set_err(CSGPU_E_HIP, "root propagate: %s", hipGetErrorString(e));
    if (rc == CSGPU_OK && res.status >= 0 && !conv) {
      hipLaunchKernelGGL(cs_propagate_sweeps, dim3(1), dim3(CS_BLOCK), lds, 0, tab, d_in, d_out, d_res, max_rounds, 1, d_conv);
      if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess ||
          (e = hipMemcpy(&res, d_res, sizeof res, hipMemcpyDeviceToHost)) != hipSuccess)
        rc = set_err(CSGPU_E_HIP, "root propagate (sequential sweeps): %s", hipGetErrorString(e));
    }
    if (rc == CSGPU_OK && (e = hipMemcpy(h->dom, d_out, (size_t)h->n_vars * sizeof(cs_val), hipMemcpyDeviceToHost)) != hipSuccess)
      rc = set_err(CSGPU_E_HIP, "root propagate: %s", hipGetErrorString(e));
    if (rc != CSGPU_OK) { /* reported below */ }
    else {
      *status = res.status < 0 ? -1 : res.props;
      if (rounds != NULL) *rounds = res.rounds;
    }
  }
  (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_res); (void)hipFree(d_conv);
  free_tables(&own);
  cs_dev_image_free(g);
  return rc;
}

extern "C" int csgpu_model_normalize(csgpu_model *m) {
  if (m == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (m->from_dump) return set_err(CSGPU_E_STATE, "a dumped model is already normalised");
  if (m->finalized) return set_err(CSGPU_E_STATE, "model is already finalized");
  if (cs_model_normalize(m->host) < 0) return set_err(CSGPU_E_STATE, "model has no root");
  return CSGPU_OK;
}

/* the model rewritten for the subtree below `state` -- a copy whose root domains are `state`, ready for
 * csgpu_model_normalize (which folds what the prefix has decided: normalize.c:67-75 replaces every subtree that now
 * evaluates to a value by that value, neutral elements and satisfied clauses drop out) and csgpu_model_finalize (which
 * leaves clauses that are true on the whole of `state` out of the device tables).  The reference does this inside the
 * search, clause by clause (normalize + patch at the end of propagate_clauses, propagate.c:521-535, undone on
 * backtracking); here it is a host-side pre-pass per subtree, as the survey puts it. */
extern "C" int csgpu_model_specialize(const csgpu_model *m, const csgpu_val *state, csgpu_model **out) {
  if (m == NULL || state == NULL || out == NULL) return set_err(CSGPU_E_ARG, "null argument");
  const cs_model *h = m->host;
  if (h->root < 0) return set_err(CSGPU_E_STATE, "model has no root");
  for (int32_t v = 0; v < h->n_vars; v++) {
    if (state[v].lo > state[v].hi) return set_err(CSGPU_E_ARG, "variable %d: empty interval", v);
    if (state[v].lo < h->dom[v].lo || state[v].hi > h->dom[v].hi)
      return set_err(CSGPU_E_ARG, "variable %d: [%d, %d] is not inside the model's [%d, %d]", v, state[v].lo, state[v].hi,
                     h->dom[v].lo, h->dom[v].hi);
  }
  cs_model *copy = cs_model_clone(h);
  if (copy == NULL) return set_err(CSGPU_E_LIMIT, "out of memory");
  memcpy(copy->dom, state, (size_t)h->n_vars * sizeof(cs_val));
  return wrap_model(copy, 0, out);
}

extern "C" int csgpu_model_add_conflict(csgpu_model *m, int32_t count, const int32_t *vars, const int32_t *values) {
  if (m == NULL || count < 1 || vars == NULL || values == NULL) return set_err(CSGPU_E_ARG, "bad argument");
  cs_model *h = m->host;
  if (h->root < 0) return set_err(CSGPU_E_STATE, "model has no root");
  if (count + 1 > CS_MAX_TREE_NODES) return set_err(CSGPU_E_LIMIT, "a conflict of %d elements, device limit is %d", count, CS_MAX_TREE_NODES - 1);
  /* a finalized model is finalized again below, which frees every device table: a search engine built on the model
   * (its captured hipGraphs, its kernels' arguments) would go on using the freed pointers */
  if (m->finalized && m->engines > 0)
    return set_err(CSGPU_E_STATE, "%d search engine(s) hold the model's device tables: free them before adding a clause", m->engines);
  int32_t *terms = (int32_t *)malloc((size_t)count * sizeof(int32_t));
  if (terms == NULL) return set_err(CSGPU_E_LIMIT, "out of memory");
  for (int32_t i = 0; i < count; i++) {
    if (vars[i] < 0 || vars[i] >= h->n_vars) {
      free(terms);
      return set_err(CSGPU_E_ARG, "conflict element %d: no such variable", i);
    }
    terms[i] = h->var_node[vars[i]];
  }
  const int32_t node = cs_model_add_confl(h, terms, values, count);
  free(terms);
  if (cs_model_append_clause(h, node) != 0) return set_err(CSGPU_E_ARG, "conflict clause could not be indexed");
  /* the device tables are immutable images: a finalized model is finalized again (O(model) per clause; learnt
   * clauses arrive once per failed node of a host-driven search, which costs a launch and a round trip anyway) */
  return m->finalized ? csgpu_model_finalize(m) : CSGPU_OK;
}

extern "C" int csgpu_model_eval_clauses_host(csgpu_model *m, csgpu_val *vals) {
  if (m == NULL || vals == NULL) return set_err(CSGPU_E_ARG, "null argument");
  quiesce_servers();
  cs_model *h = m->host;
  if (h->root < 0) return set_err(CSGPU_E_STATE, "model has no root");
  if (!m->from_dump && cs_model_index(h) != 0) return set_err(CSGPU_E_ARG, "%s", h->err);
  if (h->n_clauses == 0) return CSGPU_OK;
  char err[200];
  cs_dev_image *g = cs_dev_image_build(h, 0, NULL, err, sizeof err);
  if (g == NULL) return set_err(CSGPU_E_LIMIT, "%s", err);
  dev_tables_owner own;
  cs_tables tab;
  int rc = upload_image(g, &own, &tab);
  cs_val *d_state = NULL, *d_vals = NULL;
  const size_t lds = (size_t)h->n_vars * sizeof(cs_val) + 16;
  hipError_t e = hipSuccess;
  if (rc == CSGPU_OK) rc = lds_limit(lds, (const void *)cs_eval_clauses);
  if (rc == CSGPU_OK &&
      ((e = hipMalloc((void **)&d_state, (size_t)(h->n_vars ? h->n_vars : 1) * sizeof(cs_val))) != hipSuccess ||
       (e = hipMalloc((void **)&d_vals, (size_t)h->n_clauses * sizeof(cs_val))) != hipSuccess ||
       (e = hipMemcpy(d_state, h->dom, (size_t)h->n_vars * sizeof(cs_val), hipMemcpyHostToDevice)) != hipSuccess))
    rc = set_err(CSGPU_E_HIP, "eval: %s", hipGetErrorString(e));
  if (rc == CSGPU_OK) {
    unsigned blocks = (unsigned)((h->n_clauses + CS_BLOCK - 1) / CS_BLOCK);
    if (blocks > 1024u) blocks = 1024u;
    hipLaunchKernelGGL(cs_eval_clauses, dim3(blocks), dim3(CS_BLOCK), lds, 0, tab, d_state, d_vals);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess ||
        (e = hipMemcpy(vals, d_vals, (size_t)h->n_clauses * sizeof(cs_val), hipMemcpyDeviceToHost)) != hipSuccess)
      rc = set_err(CSGPU_E_HIP, "eval: %s", hipGetErrorString(e));
  }
  (void)hipFree(d_state); (void)hipFree(d_vals);
  free_tables(&own);
  cs_dev_image_free(g);
  return rc;
}

/* instantiation of the LDS-resident kernel for an entry width and a prefetch depth
 * R = ceil(n_vars / 64) rounded up to a power of two (at most 16: larger states load their tail in place) */
static const void *ne_lds_kernel(int width, int n_vars, int adj_global) {
  /* the largest instantiated depth that is at most ceil(n_vars / 64): all its strides but the last are full (the kernel
   * relies on that), a longer state loads its tail in place */
  const int strides = (n_vars + CS_WAVE - 1) / CS_WAVE;
  int r = strides >= 16 ? 16 : (strides >= 8 ? 8 : (strides >= 4 ? 4 : (strides >= 2 ? 2 : 1)));
  /* 577 to 1023 variables (a 25x25 sudoku has 625): ten strides in registers */
  if (strides >= 10 && strides < 16 && !adj_global)
    return width == 2 ? (const void *)cs_propagate_ne_lds<unsigned short, 10, 1, true>
                      : (const void *)cs_propagate_ne_lds<unsigned int, 10, 1, true>;
#define CS_PICK_U(E, RR) return adj_global ? (const void *)cs_propagate_ne_lds<E, RR, 1, false> : (const void *)cs_propagate_ne_lds<E, RR, 1, true>;
#define CS_PICK(E)                                                                                 \
  switch (r) {                                                                                     \
  case 1: CS_PICK_U(E, 1)                                                                          \
  case 2: CS_PICK_U(E, 2)                                                                          \
  case 4: CS_PICK_U(E, 4)                                                                          \
  case 8: CS_PICK_U(E, 8)                                                                          \
  default: CS_PICK_U(E, 16)                                                                        \
  }
  if (width == 2) { CS_PICK(unsigned short) }
  CS_PICK(unsigned int)
#undef CS_PICK
#undef CS_PICK_U
}

static const void *ne_bitset_kernel(int width, int fw, int n_vars) {
  /* prefetch depth R = ceil(n_vars/64) when that is 1, 2 or 4 (states of up to 256 variables), or 10 with
   * one set word per variable (up to 640 variables: a 25x25 sudoku's next state travels in 40 VGPRs) */
  const int chunks = (n_vars + CS_WAVE - 1) / CS_WAVE;
  int r = chunks <= 1 ? 1 : (chunks <= 2 ? 2 : (chunks <= 4 ? 4 : (chunks <= 10 && fw == 1 ? 10 : 0)));
#define CS_PICK_R(E, F)                                                                            \
  switch (r) {                                                                                     \
  case 1: return (const void *)cs_propagate_ne_bitset<E, F, 1>;                                    \
  case 2: return (const void *)cs_propagate_ne_bitset<E, F, 2>;                                    \
  case 4: return (const void *)cs_propagate_ne_bitset<E, F, 4>;                                    \
  case 10: return (const void *)cs_propagate_ne_bitset<E, 1, 10>;                                  \
  default: return (const void *)cs_propagate_ne_bitset<E, F, 0>;                                   \
  }
#define CS_PICK(E)                                                                                 \
  switch (fw) {                                                                                    \
  case 1: CS_PICK_R(E, 1)                                                                          \
  case 2: CS_PICK_R(E, 2)                                                                          \
  default: CS_PICK_R(E, 4)                                                                         \
  }
  if (width == 2) { CS_PICK(unsigned short) }
  CS_PICK(unsigned int)
#undef CS_PICK
#undef CS_PICK_R
}

/* register-resident forbidden-set kernel: entry width, set words, variables per lane; the FAST
 * instantiation (n_vars a multiple of 64 that fills the lanes, both set buffers) keeps D nodes in flight */
static const void *ne_regs_kernel(int width, int fw, int n_vars, int fast, int sets_only) {
  const int r = cs_dense_strides(n_vars);
#define CS_PICK_D(E, F, RR)                                                                        \
  if (sets_only)                                                                                   \
    return fast ? (const void *)cs_propagate_ne_regs<E, F, RR, 2, true, true>                       \
                : (const void *)cs_propagate_ne_regs<E, F, RR, 1, false, true>;                     \
  return fast ? (const void *)cs_propagate_ne_regs<E, F, RR, 2, true, false>                        \
              : (const void *)cs_propagate_ne_regs<E, F, RR, 1, false, false>;
#define CS_PICK_R(E, F)                                                                            \
  switch (r) {                                                                                     \
  case 1: CS_PICK_D(E, F, 1)                                                                       \
  case 2: CS_PICK_D(E, F, 2)                                                                       \
  default: CS_PICK_D(E, F, 4)                                                                      \
  }
#define CS_PICK(E)                                                                                 \
  switch (fw) {                                                                                    \
  case 1: CS_PICK_R(E, 1)                                                                          \
  case 2: CS_PICK_R(E, 2)                                                                          \
  default: CS_PICK_R(E, 4)                                                                         \
  }
  if (width == 1) { CS_PICK(unsigned char) }
  CS_PICK(unsigned short)
#undef CS_PICK
#undef CS_PICK_R
#undef CS_PICK_D
}

/* kernel 7 (cs_shave.hip.h): interval states only; entry width, variables per lane, slots per pair known at
 * compile time when 1 or 3, FULL when the variables fill the lanes */
static const void *ne_shave_kernel(int width, int n_vars, int slots, int full) {
  const int r = cs_dense_strides(n_vars);
  const int sl = slots == 1 ? 1 : (slots == 3 ? 3 : 0);
#define CS_PICK_F(E, RR, SS)                                                                       \
  return full ? (const void *)cs_propagate_ne_shave<E, RR, SS, true>                                \
              : (const void *)cs_propagate_ne_shave<E, RR, SS, false>;
#define CS_PICK_S(E, RR)                                                                           \
  switch (sl) {                                                                                    \
  case 1: CS_PICK_F(E, RR, 1)                                                                      \
  case 3: CS_PICK_F(E, RR, 3)                                                                      \
  default: CS_PICK_F(E, RR, 0)                                                                     \
  }
#define CS_PICK(E)                                                                                 \
  switch (r) {                                                                                     \
  case 1: CS_PICK_S(E, 1)                                                                          \
  case 2: CS_PICK_S(E, 2)                                                                          \
  default: CS_PICK_S(E, 4)                                                                         \
  }
  if (width == 1) { CS_PICK(unsigned char) }
  CS_PICK(unsigned short)
#undef CS_PICK
#undef CS_PICK_S
#undef CS_PICK_F
}

/* its tracing variant for single nodes (guarded lanes; the slot count a constant when 1 or 3: with the run-time loop
 * the six LDS reads of a row operation are waited for one by one, which is the latency of a single wavefront) */
static const void *ne_shave_trace_kernel(int width, int n_vars, int slots) {
  const int r = cs_dense_strides(n_vars);
  const int sl = slots == 1 ? 1 : (slots == 3 ? 3 : 0);
#define CS_PICK_S(E, RR)                                                                           \
  switch (sl) {                                                                                    \
  case 1: return (const void *)cs_propagate_ne_shave<E, RR, 1, false, true>;                        \
  case 3: return (const void *)cs_propagate_ne_shave<E, RR, 3, false, true>;                        \
  default: return (const void *)cs_propagate_ne_shave<E, RR, 0, false, true>;                       \
  }
#define CS_PICK(E)                                                                                 \
  switch (r) {                                                                                     \
  case 1: CS_PICK_S(E, 1)                                                                          \
  case 2: CS_PICK_S(E, 2)                                                                          \
  default: CS_PICK_S(E, 4)                                                                         \
  }
  if (width == 1) { CS_PICK(unsigned char) }
  CS_PICK(unsigned short)
#undef CS_PICK
#undef CS_PICK_S
}

/* kernel 5: kernel 4 for small models, 64 / n_vars (2 or 4) nodes per wave; needs the 8-bit dense table (its
 * 16-bit LDS copy is relative to the pushing variable, cs_kernels.hip.h) */
static int packed_nodes_per_wave(int fw, int n_vars, int dense_width) {
  return fw == 1 && dense_width == 1 && n_vars <= 32 ? (n_vars <= 16 ? 4 : 2) : 0;
}

/* kernel 5 and the step kernels built on it: 64 / n_vars nodes per wave (4 or 2), set words per variable, three slots */
#define CS_PACKED_PICKER(NAME, KERNEL)                                                                 \
  static const void *NAME(int n_vars, int nw, int s3) {                                                \
    if (n_vars <= 16) {                                                                                \
      if (nw == 1) return s3 ? (const void *)KERNEL<4, 1, true> : (const void *)KERNEL<4, 1, false>;    \
      return s3 ? (const void *)KERNEL<4, 2, true> : (const void *)KERNEL<4, 2, false>;                 \
    }                                                                                                  \
    if (nw == 1) return s3 ? (const void *)KERNEL<2, 1, true> : (const void *)KERNEL<2, 1, false>;      \
    return s3 ? (const void *)KERNEL<2, 2, true> : (const void *)KERNEL<2, 2, false>;                   \
  }
CS_PACKED_PICKER(ne_packed_kernel, cs_propagate_ne_packed)
CS_PACKED_PICKER(step_packed_kernel, cs_step_packed)
CS_PACKED_PICKER(step_import_kernel, cs_step_import)
#undef CS_PACKED_PICKER

/* ---- cs_step.hip.h: one level of the search tree per launch ---- */
static const void *step_shave_kernel(int width, int n_vars, int slots, int full) {
#define CS_PICK_S(E, R)                                                                                   \
  if (slots == 1) return full ? (const void *)cs_step_shave<E, R, 1, true> : (const void *)cs_step_shave<E, R, 1, false>; \
  if (slots == 3) return full ? (const void *)cs_step_shave<E, R, 3, true> : (const void *)cs_step_shave<E, R, 3, false>; \
  return full ? (const void *)cs_step_shave<E, R, 0, true> : (const void *)cs_step_shave<E, R, 0, false>;
#define CS_PICK(E)                                                                                 \
  switch (cs_dense_strides(n_vars)) {                                                              \
  case 1: CS_PICK_S(E, 1)                                                                          \
  case 2: CS_PICK_S(E, 2)                                                                          \
  default: CS_PICK_S(E, 4)                                                                         \
  }
  if (width == 1) { CS_PICK(unsigned char) }
  CS_PICK(unsigned short)
#undef CS_PICK
#undef CS_PICK_S
}

/* ---- cs_dive.hip.h: a depth-first search per wave (csgpu_solve_many); the slot count is always a run-time value ---- */
static const void *dive_kernel(int family, int width, int n_vars, int set_words) {
  const int r = cs_dense_strides(n_vars);
  if (MANY_BY_ALLOWED(family)) { /* set_words: 1 or 4 words of 32 allowed values per variable */
#define CS_PICK_R(K, E, NW) (r == 1 ? (const void *)K<E, 1, NW> : r == 2 ? (const void *)K<E, 2, NW> : (const void *)K<E, 4, NW>)
#define CS_PICK_E(K, NW) (width == 1 ? CS_PICK_R(K, unsigned char, NW) : CS_PICK_R(K, unsigned short, NW))
#define CS_PICK(K) return set_words == 1 ? CS_PICK_E(K, 1) : CS_PICK_E(K, 4);
    if (family == MANY_ALLOWED) { CS_PICK(cs_dive_allowed) }
    if (family == MANY_ALLOWED_CK) { CS_PICK(cs_dive_allowed_resume) }           /* csgpu_solve_many_allowed_checkpointed / _resume */
    if (family == MANY_ALLOWED_UPTO_CK) { CS_PICK(cs_dive_allowed_upto_resume) } /* and up to k */
    CS_PICK(cs_dive_allowed_upto)
#undef CS_PICK
#undef CS_PICK_E
#undef CS_PICK_R
  }
#define CS_PICK_R(K, E) (r == 1 ? (const void *)K<E, 1> : r == 2 ? (const void *)K<E, 2> : (const void *)K<E, 4>)
#define CS_PICK(K) return width == 1 ? CS_PICK_R(K, unsigned char) : CS_PICK_R(K, unsigned short);
  switch (family) {
  case MANY_CK: CS_PICK(cs_dive_resume)       /* with checkpoints (csgpu_solve_many_checkpointed / _resume) */
  case MANY_UPTO: CS_PICK(cs_dive_upto)       /* leaving at the k-th solution (csgpu_solve_many_upto and its two checkpoint calls) */
  case MANY_RESTART: CS_PICK(cs_dive_restart) /* ANY with a seeded value order and Luby restarts (csgpu_solve_many_restarts) */
  case MANY_STREAM: CS_PICK(cs_dive_stream)   /* ALL, every solution appended to a shared stream (csgpu_solve_many_stream) */
  default: CS_PICK(cs_dive_shave)
  }
#undef CS_PICK
#undef CS_PICK_R
}

/* ---- cs_walk.hip.h: a depth-first search per wave on kernel 6's fixpoint (csgpu_solve_many_clauses); `cpl`: kernel 6's
 * clauses per lane, `tree`: some adjacency entry is a tree clause ---- */
static const void *walk_kernel(int family, int cpl, int tree) {
#define CS_PICK_T(K, CPL) (tree ? (const void *)K<CPL, true> : (const void *)K<CPL, false>)
#define CS_PICK(K) return cpl == 1 ? CS_PICK_T(K, 1) : (cpl == 2 ? CS_PICK_T(K, 2) : (cpl == 4 ? CS_PICK_T(K, 4) : CS_PICK_T(K, 8)));
  switch (family) {
  case WALK_CK: CS_PICK(cs_walk_resume)       /* with checkpoints (csgpu_solve_many_clauses_checkpointed / _resume) */
  case WALK_UPTO: CS_PICK(cs_walk_upto)       /* leaving at the k-th solution (csgpu_solve_many_clauses_upto and its two checkpoint calls) */
  case WALK_RESTART: CS_PICK(cs_walk_restart) /* ANY with a seeded value order and Luby restarts (csgpu_solve_many_clauses_restarts) */
  case WALK_STREAM: CS_PICK(cs_walk_stream)   /* ALL, every solution appended to a shared stream (csgpu_solve_many_clauses_stream) */
  case WALK_FROM: CS_PICK(cs_walk_from)       /* MIN / MAX from a start incumbent (csgpu_solve_many_clauses_from / _from_resume) */
  case WALK_ORDER: CS_PICK(cs_walk_order)     /* the five variable orders, interval halving (csgpu_solve_many_clauses_ordered) */
  case WALK_ORDER_CK: CS_PICK(cs_walk_order_resume) /* that walk with checkpoints (csgpu_solve_many_clauses_ordered_checkpointed / _resume) */
  case WALK_ORDER_FROM: CS_PICK(cs_walk_order_from) /* and from a start incumbent (csgpu_solve_many_clauses_ordered_from / _from_resume) */
  default: CS_PICK(cs_walk_clauses)
  }
#undef CS_PICK
#undef CS_PICK_T
}

/* ---- the resident single-node server (cs_shave.hip.h) ---- */
static const void *shave_server_kernel(int width, int n_vars, int slots) {
  const int r = cs_dense_strides(n_vars);
  const int sl = slots == 1 ? 1 : (slots == 3 ? 3 : 0);
#define CS_PICK_S(E, RR)                                                                           \
  switch (sl) {                                                                                    \
  case 1: return (const void *)cs_shave_server<E, RR, 1>;                                           \
  case 3: return (const void *)cs_shave_server<E, RR, 3>;                                           \
  default: return (const void *)cs_shave_server<E, RR, 0>;                                          \
  }
#define CS_PICK(E)                                                                                 \
  switch (r) {                                                                                     \
  case 1: CS_PICK_S(E, 1)                                                                          \
  case 2: CS_PICK_S(E, 2)                                                                          \
  default: CS_PICK_S(E, 4)                                                                         \
  }
  if (width == 1) { CS_PICK(unsigned char) }
  CS_PICK(unsigned short)
#undef CS_PICK
#undef CS_PICK_S
}

/* LDS of a step workgroup of `waves` waves: the 16-bit table, then per wave the parent slots and the child queue */
static size_t step_packed_lds(const csgpu_model *m, int waves) {
  return ((2 * m->dense_bytes + 15) & ~(size_t)15) + (size_t)waves * ((1 + m->packed_nw) * 256 + CS_STEP_QN) * sizeof(unsigned);
}

/* ---- finalize ---------------------------------------------------------------------- */

/* resident workgroups per CU of `lds` bytes and `waves` waves each: LDS- and wave-slot-limited (32 waves per CU) */
static int resident_per_cu(size_t lds, int waves) {
  size_t wgs = lds > 0 ? CS_CU_LDS / lds : (size_t)32;
  if (wgs > (size_t)(32 / waves)) wgs = (size_t)(32 / waves);
  return (int)wgs;
}

/* nodes per chunk: `csz` halved while the batch would make fewer than `min_chunks` chunks */
static int shrink_chunk(int csz, int64_t batch, int64_t min_chunks) {
  while (csz > 1 && (batch + csz - 1) / csz < min_chunks) csz >>= 1;
  return csz;
}

/* plan `fn` with `lds` bytes and `waves` waves per workgroup, and set its LDS attribute */
static int plan_kernel(cs_planned *p, const void *fn, size_t lds, int waves) {
  const int rc = lds_limit(lds, fn);
  if (rc != CSGPU_OK) return rc;
  p->fn = fn;
  p->lds = lds;
  p->waves = waves;
  p->per_cu = resident_per_cu(lds, waves);
  return CSGPU_OK;
}

extern "C" int csgpu_model_build_tables(csgpu_model *m) {
  if (m == NULL) return set_err(CSGPU_E_ARG, "null argument");
  cs_model *h = m->host;
  int32_t ub = cs_model_first_unbounded(h);
  if (ub >= 0) return set_err(CSGPU_E_UNBOUNDED, "unbounded variable: %s", h->names[ub]);
  if (!m->from_dump && cs_model_index(h) != 0) return set_err(CSGPU_E_ARG, "%s", h->err);
  cs_dev_image_free(m->img);
  m->img = NULL;
  m->finalized = 0;
  char err[200];
  m->img = cs_dev_image_build(h, 1, NULL, err, sizeof err);
  if (m->img == NULL) return set_err(CSGPU_E_LIMIT, "%s", err);
  const size_t slice = (size_t)h->n_vars * sizeof(cs_val) + 2 * (size_t)((h->n_vars + 31) / 32) * sizeof(unsigned);
  m->slice = (slice + 15) & ~(size_t)15;
  return CSGPU_OK;
}

/* Upload the tables.  Clauses that already evaluate to true in the root state are entailed for the whole search:
 * evaluate every clause once on the device and drop those from the tables. */
static int drop_entailed_clauses(csgpu_model *m) {
  cs_model *h = m->host;
  dev_tables_owner own;
  int rc = upload_image(m->img, &own, &m->tab);
  if (rc == CSGPU_OK && h->n_clauses > 0 && !m->not_root) {
    cs_val *d_state = NULL, *d_vals = NULL;
    const size_t lds0 = (size_t)h->n_vars * sizeof(cs_val) + 16;
    cs_val *vals = (cs_val *)malloc((size_t)h->n_clauses * sizeof(cs_val));
    unsigned char *entailed = (unsigned char *)calloc((size_t)h->n_clauses, 1);
    hipError_t e = hipSuccess;
    rc = lds_limit(lds0, (const void *)cs_eval_clauses);
    if (rc == CSGPU_OK &&
        ((e = hipMalloc((void **)&d_state, (size_t)(h->n_vars ? h->n_vars : 1) * sizeof(cs_val))) != hipSuccess ||
         (e = hipMalloc((void **)&d_vals, (size_t)h->n_clauses * sizeof(cs_val))) != hipSuccess ||
         (e = hipMemcpy(d_state, h->dom, (size_t)h->n_vars * sizeof(cs_val), hipMemcpyHostToDevice)) != hipSuccess))
      rc = set_err(CSGPU_E_HIP, "finalize: %s", hipGetErrorString(e));
    if (rc == CSGPU_OK) {
      unsigned blocks = (unsigned)((h->n_clauses + CS_BLOCK - 1) / CS_BLOCK);
      if (blocks > 1024u) blocks = 1024u;
      hipLaunchKernelGGL(cs_eval_clauses, dim3(blocks), dim3(CS_BLOCK), lds0, 0, m->tab, d_state, d_vals);
      if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess ||
          (e = hipMemcpy(vals, d_vals, (size_t)h->n_clauses * sizeof(cs_val), hipMemcpyDeviceToHost)) != hipSuccess)
        rc = set_err(CSGPU_E_HIP, "finalize: %s", hipGetErrorString(e));
    }
    (void)hipFree(d_state); (void)hipFree(d_vals);
    if (rc == CSGPU_OK) {
      int any = 0;
      for (int32_t c = 0; c < h->n_clauses; c++)
        if (m->img->clause[4 * c] != CS_CL_SKIP && cs_is_true(vals[c])) { entailed[c] = 1; any = 1; }
      if (any) {
        free_tables(&own);
        memset(&own, 0, sizeof own);
        cs_dev_image_free(m->img);
        char err2[200];
        m->img = cs_dev_image_build(h, 1, entailed, err2, sizeof err2);
        if (m->img == NULL) rc = set_err(CSGPU_E_LIMIT, "%s", err2);
        else rc = upload_image(m->img, &own, &m->tab);
      }
    }
    free(vals); free(entailed);
  }
  m->d_adj_off = own.adj_off; m->d_adj = own.adj; m->d_clause = own.clause; m->d_clause_by_kind = own.clause_by_kind;
  m->d_tree_off = own.tree_off; m->d_tnode = own.tnode; m->d_tkid = own.tkid; m->d_tree_want = own.tree_want;
  m->d_lit = own.lit;
  return rc;
}

/* dynamic LDS of a cs_walk_wide workgroup: the staged block -- the clause records, then two literal records per
 * two-literal disjunction, 16 bytes each -- and behind it the slices of its waves (kernel 6's: n intervals and the flag) */
static size_t many_wide_lds(int n_vars, int n_clauses, int n_lits) {
  const size_t slice = ((size_t)n_vars * sizeof(cs_val) + 16 + 15) & ~(size_t)15;
  return ((size_t)n_clauses + (size_t)n_lits) * 16 + slice * CS_WAVES_PER_BLOCK;
}

/* kernels every model runs: the general kernel (1) and its tracing variant, the clause-resident kernel (6), the
 * clause evaluation */
static int plan_general(csgpu_model *m) {
  const cs_model *h = m->host;
  const size_t slice = (size_t)h->n_vars * sizeof(cs_val) + 2 * (size_t)m->tab.n_words * sizeof(unsigned);
  m->slice = (slice + 15) & ~(size_t)15;
  m->has_tree_adj = 0;
  for (int32_t i = 0; i < m->img->n_adj; i++)
    if (m->img->adj[2 * i] < 0 && m->img->adj[2 * i + 1] == 0) { m->has_tree_adj = 1; break; }
  /* small tables travel into LDS with every workgroup of the general kernel */
  const size_t tb = ((((size_t)h->n_vars + 1) * 4 + 15) & ~(size_t)15) + (((size_t)m->img->n_adj * 8 + 15) & ~(size_t)15) +
                    (((size_t)m->img->n_lits * 16 + 15) & ~(size_t)15);
  m->k1_tab_bytes = (tb <= 32u * 1024u && m->img->n_adj > 0) ? tb : 0;
  const void *k1 = m->has_tree_adj ? (m->k1_tab_bytes ? (const void *)cs_propagate_events<true, true>
                                                      : (const void *)cs_propagate_events<true, false>)
                                   : (m->k1_tab_bytes ? (const void *)cs_propagate_events<false, true>
                                                      : (const void *)cs_propagate_events<false, false>);
  int rc;
  if ((rc = plan_kernel(&m->plan.events, k1, m->slice * CS_WAVES_PER_BLOCK + m->k1_tab_bytes, CS_WAVES_PER_BLOCK)))
    return rc;
  if (m->plan.events.per_cu < 1) m->plan.events.per_cu = 1;
  if ((rc = lds_limit((size_t)h->n_vars * sizeof(cs_val) + 16, (const void *)cs_eval_root))) return rc;
  if ((rc = lds_limit((size_t)h->n_vars * sizeof(cs_val) + 16, (const void *)cs_eval_clauses))) return rc;
  if ((rc = plan_kernel(&m->plan.traced, (const void *)cs_propagate_events<true, false, true>, m->slice * CS_WAVES_PER_BLOCK,
                        CS_WAVES_PER_BLOCK)))
    return rc;
  /* kernel 6: launched without an LDS attribute; its grid is eight workgroups per CU, four times over */
  const int per = (m->img->n_clauses + CS_WAVE - 1) / CS_WAVE; /* clauses per lane: 1, 2, 4, 8 for at most 512 clauses */
  m->plan.rounds_cpl = m->img->n_clauses <= 0 || per > 8 ? 0 : (per <= 1 ? 1 : (per <= 2 ? 2 : (per <= 4 ? 4 : 8)));
  if (m->plan.rounds_cpl) {
#define CS_PICK6(CPL)                                                                              \
  m->plan.rounds.fn = m->has_tree_adj ? (const void *)cs_propagate_clause_rounds<CPL, true>         \
                                      : (const void *)cs_propagate_clause_rounds<CPL, false>
    switch (m->plan.rounds_cpl) {
    case 1: CS_PICK6(1); break;
    case 2: CS_PICK6(2); break;
    case 4: CS_PICK6(4); break;
    default: CS_PICK6(8); break;
    }
#undef CS_PICK6
    m->plan.rounds.lds = ((((size_t)h->n_vars * sizeof(cs_val) + 16 + 15) & ~(size_t)15)) * CS_WAVES_PER_BLOCK;
    m->plan.rounds.waves = CS_WAVES_PER_BLOCK;
    m->plan.rounds.per_cu = 8;
    /* the cs_walk_* kernels: kernel 6's slices, each its own registers; planned when a workgroup's fit a CU
     * (csgpu_solve_many_clauses says so otherwise) */
    if (m->plan.rounds.lds <= CS_CU_LDS) {
      for (int family = 0; family < WALK_FAMILIES; family++) {
        cs_planned *k = &m->plan.walk[family];
        if ((rc = plan_kernel(k, walk_kernel(family, m->plan.rounds_cpl, m->has_tree_adj), m->plan.rounds.lds, CS_WAVES_PER_BLOCK)))
          return rc;
        /* persistent waves: no more workgroups than stay resident with the instantiation's registers and scratch */
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k->fn, CS_BLOCK, k->lds) == hipSuccess && occ >= 1 && occ < k->per_cu)
          k->per_cu = occ;
        if (k->per_cu < 1) k->per_cu = 1;
      }
      if ((rc = upload(h->dom, (size_t)h->n_vars * sizeof(cs_val), (int **)&m->d_walk_root))) return rc;
    }
  }
  /* the two cs_walk_wide kernels: the records in LDS, so no clause count of their own -- every model with a clause whose
   * staged block and slices fit a CU, those of at most 512 clauses as well */
  const size_t wide = many_wide_lds(h->n_vars, m->tab.n_clauses, m->tab.n_lits);
  if (m->tab.n_clauses > 0 && wide <= CS_CU_LDS) {
    for (int family = WALK_WIDE; family <= WALK_WIDE_CK; family++) {
      cs_planned *k = &m->plan.walk[family];
      const void *fn = family == WALK_WIDE ? (m->has_tree_adj ? (const void *)cs_walk_wide<true> : (const void *)cs_walk_wide<false>)
                                           : (m->has_tree_adj ? (const void *)cs_walk_wide_resume<true>
                                                              : (const void *)cs_walk_wide_resume<false>);
      if ((rc = plan_kernel(k, fn, wide, CS_WAVES_PER_BLOCK))) return rc;
      int occ = 0; /* persistent waves, as the other walks: what stays resident with its registers, scratch and LDS */
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k->fn, CS_BLOCK, k->lds) == hipSuccess && occ >= 1 && occ < k->per_cu)
        k->per_cu = occ;
      if (k->per_cu < 1) k->per_cu = 1;
    }
    if (m->d_walk_root == NULL && (rc = upload(h->dom, (size_t)h->n_vars * sizeof(cs_val), (int **)&m->d_walk_root))) return rc;
  }
  m->plan.max_width = 2;
  for (int32_t v = 0; v < h->n_vars; v++) {
    const int64_t w = (int64_t)h->dom[v].hi - (int64_t)h->dom[v].lo + 1;
    if (w > m->plan.max_width) m->plan.max_width = w > 0x7fffffff ? 0x7fffffff : (int)w;
  }
  return CSGPU_OK;
}

/* LDS-resident kernel (2): adj_off + packed adjacency + one slice per wave must fit in a CU's LDS */
static int plan_lds_resident(csgpu_model *m) {
  const cs_model *h = m->host;
  if (m->img->packed_width == 0) return CSGPU_OK;
  const size_t off_bytes = (((size_t)h->n_vars * 2 * sizeof(int)) + 15) & ~(size_t)15;
  const size_t adj_bytes = (((size_t)m->img->n_adj * (size_t)m->img->packed_width) + 15) & ~(size_t)15;
  const size_t lds_slice = ((size_t)h->n_vars * sizeof(cs_val) + (2 * (size_t)m->tab.n_words + 1) * sizeof(unsigned) + 15) & ~(size_t)15;
  m->lds_adj_global = 0;
  /* as many waves as fit next to the lists (not only 16, 8 or 4: the 25x25 sudoku's lists leave room for fifteen
   * slices, and with eight its nodes' chains of dependent steps had two waves per SIMD to hide behind) */
  int waves_max = 16, waves = 0;
  size_t bytes = 0;
  { const char *e = getenv("CSGPU_K2_WAVES"); if (e != NULL && atoi(e) >= 4 && atoi(e) <= 16) waves_max = atoi(e); } /* measurement override */
  for (int w = waves_max; w >= 4; w--) {
    const size_t need = off_bytes + adj_bytes + (size_t)w * lds_slice;
    if (need <= CS_CU_LDS) {
      waves = w;
      bytes = need;
      break;
    }
  }
  const char *force = getenv("CSGPU_K2_ADJ"); /* "global": measurement override */
  const int want_global = force != NULL && force[0] == 'g';
  if (want_global && 8 * lds_slice <= CS_CU_LDS) {
    /* the lists in device memory (L2-resident) and LDS for the node slices only: 24 waves per CU instead of 16 on
     * the 25x25 sudoku network -- and 1.23 ms instead of 0.75 ms for 2^18 nodes: the two-byte gathers through L2
     * cost more than the extra waves hide.  Kept for measurements; never chosen automatically. */
    m->lds_adj_global = 1;
    waves = 8;
    bytes = 8 * lds_slice;
  }
  { const char *e = getenv("CSGPU_K2_CSZ"); m->k2_csz = e != NULL && atoi(e) >= 1 && atoi(e) <= CS_CHUNK ? atoi(e) : 0; } /* measurement override */
  if (!waves) return CSGPU_OK;
  int rc;
  if ((rc = upload(m->img->adj_packed, (size_t)m->img->n_adj * (size_t)m->img->packed_width, (int **)&m->d_adj_packed)))
    return rc;
  if ((rc = plan_kernel(&m->plan.lds, ne_lds_kernel(m->img->packed_width, h->n_vars, m->lds_adj_global), bytes, waves)))
    return rc;
  if (m->plan.lds.per_cu < 1) m->plan.lds.per_cu = 1;
  return CSGPU_OK;
}

/* forbidden-set kernel (3): additionally root intervals of at most 256 values, and only when the
 * host domains really are the root state (the bit windows are anchored at the root bounds) */
/* its shape from the host image alone: waves per workgroup (0: the model does not qualify), set words per variable and
 * LDS bytes per workgroup */
static int64_t widest_root_domain(const csgpu_model *m) {
  const cs_model *h = m->host;
  int64_t width = 1;
  for (int32_t v = 0; v < h->n_vars; v++) {
    const int64_t w = (int64_t)h->dom[v].hi - (int64_t)h->dom[v].lo + 1;
    if (w > width) width = w;
  }
  return width;
}

static int forbidden_sets_shape(const csgpu_model *m, int *fw_out, size_t *lds_out) {
  const cs_model *h = m->host;
  if (m->img->sym_width == 0 || m->not_root) return 0;
  const int64_t width = widest_root_domain(m);
  const int fw = width <= 64 ? 1 : (width <= 128 ? 2 : (width <= 256 ? 4 : 0));
  if (!fw) return 0;
  const size_t n_words = ((size_t)h->n_vars + 31) / 32; /* cs_tables.n_words */
  const size_t off_bytes = (((size_t)h->n_vars * 2 * sizeof(int)) + 15) & ~(size_t)15;
  const size_t base_bytes = (((size_t)h->n_vars * sizeof(int)) + 15) & ~(size_t)15;
  const size_t adj_bytes = (((size_t)m->img->sym_n_adj * (size_t)m->img->sym_width) + 15) & ~(size_t)15;
  const size_t sl = ((size_t)h->n_vars * sizeof(cs_val) + (size_t)h->n_vars * fw * 8 + (2 * n_words + 2) * sizeof(unsigned) + 15) &
                    ~(size_t)15;
  int waves = 16;
  for (; waves >= 1; waves--) /* as many waves as fit next to the tables */
    if (off_bytes + base_bytes + adj_bytes + (size_t)waves * sl <= CS_CU_LDS) break;
  if (waves < 1) return 0;
  *fw_out = fw;
  *lds_out = off_bytes + base_bytes + adj_bytes + (size_t)waves * sl;
  return waves;
}

static int plan_forbidden_sets(csgpu_model *m) {
  const cs_model *h = m->host;
  int fw = 0;
  size_t lds = 0;
  const int waves = forbidden_sets_shape(m, &fw, &lds);
  if (!waves) return CSGPU_OK;
  m->fb_words = fw;
  int *lo = (int *)malloc((size_t)(h->n_vars ? h->n_vars : 1) * sizeof(int));
  for (int32_t v = 0; v < h->n_vars; v++) lo[v] = h->dom[v].lo;
  int rc = upload(lo, (size_t)h->n_vars * sizeof(int), &m->d_root_lo);
  free(lo);
  if (rc) return rc;
  if ((rc = upload(m->img->sym_off, ((size_t)h->n_vars + 1) * sizeof(int), &m->d_sym_off))) return rc;
  if ((rc = upload(m->img->sym_packed, (size_t)m->img->sym_n_adj * (size_t)m->img->sym_width, (int **)&m->d_sym_packed)))
    return rc;
  if ((rc = plan_kernel(&m->plan.bitset, ne_bitset_kernel(m->img->sym_width, fw, h->n_vars), lds, waves))) return rc;
  if (m->plan.bitset.per_cu < 1) m->plan.bitset.per_cu = 1;
  return CSGPU_OK;
}

/* the dense pair table in LDS: the register-resident forbidden-set kernel (4), the interval-only kernel (7) with its
 * tracing variant, the server and cs_step_shave; kernel 7's ticket counters */
/* waves per workgroup of the kernels with the dense table in LDS, from the host image alone (0: the model has no such
 * table, or it does not fit) */
static int dense_table_waves(const csgpu_model *m, size_t *bytes_out) {
  if (m->img->dense_width == 0) return 0;
  /* the dense table must fit a CU's LDS; the workgroup size that keeps the most waves resident (32 per CU at most),
   * smaller workgroups on ties */
  const size_t bytes = (size_t)m->host->n_vars * m->img->dense_slots * m->img->dense_cols * m->img->dense_width;
  int best = 0, waves = 0;
  for (int w = 4; w <= 16; w <<= 1)
    if (resident_per_cu(bytes, w) * w > best) { best = resident_per_cu(bytes, w) * w; waves = w; }
  *bytes_out = bytes;
  return waves;
}

static int plan_dense_table(csgpu_model *m) {
  const cs_model *h = m->host;
  if (!m->fb_words) return CSGPU_OK;
  const int n = h->n_vars, width = m->img->dense_width, slots = m->img->dense_slots;
  size_t bytes = 0;
  const int waves = dense_table_waves(m, &bytes);
  if (!waves) return CSGPU_OK;
  m->dense_bytes = bytes;
  int rc;
  if ((rc = upload(m->img->dense_tab, bytes, (int **)&m->d_dense_tab))) return rc;
  for (int variant = 0; variant < 4; variant++)
    if ((rc = plan_kernel(&m->plan.regs[variant], ne_regs_kernel(width, m->fb_words, n, variant & 1, variant >> 1), bytes, waves)))
      return rc;
  m->plan.full = n == cs_dense_strides(n) * CS_WAVE;
  if ((rc = plan_kernel(&m->plan.shave, ne_shave_kernel(width, n, slots, m->plan.full), bytes, waves))) return rc;
  const size_t table = (bytes + 15) & ~(size_t)15;
  /* cs_step_shave: the table, then eight mask words per wave */
  if (table + (size_t)waves * 32 <= CS_CU_LDS &&
      (rc = plan_kernel(&m->plan.step_shave, step_shave_kernel(width, n, slots, m->plan.full), table + (size_t)waves * 32, waves)))
    return rc;
  /* the single-node kernels keep the trail in LDS after the table; the server sets its attribute when it first starts */
  if (table + CS_SHAVE_TRACE_LDS * 16 <= CS_CU_LDS) {
    if ((rc = plan_kernel(&m->plan.shave_trace, ne_shave_trace_kernel(width, n, slots), table + CS_SHAVE_TRACE_LDS * 16, waves)))
      return rc;
    m->plan.server = m->plan.shave_trace;
    m->plan.server.fn = shave_server_kernel(width, n, slots);
  }
  /* the cs_dive_* kernels: the table alone; the upper bounds of the root domains for its check of the root rows */
  const int64_t widest = widest_root_domain(m);
  for (int family = 0; family < MANY_FAMILIES; family++) {
    const int by_allowed = MANY_BY_ALLOWED(family);
    if (by_allowed && widest > CS_DIVE_ALLOWED_WIDTH) continue; /* not planned: the calls say why */
    if ((rc = plan_kernel(&m->plan.dive[family], dive_kernel(family, width, n, widest <= 32 ? 1 : 4), table, waves))) return rc;
  }
  {
    int *hi = (int *)malloc((size_t)n * sizeof(int));
    if (hi == NULL) return set_err(CSGPU_E_ARG, "out of memory");
    for (int32_t v = 0; v < n; v++) hi[v] = h->dom[v].hi;
    rc = upload(hi, (size_t)n * sizeof(int), &m->d_root_hi);
    free(hi);
    if (rc) return rc;
  }
  HIP_TRY(hipMalloc((void **)&m->d_tickets, (size_t)CS_TICKET_SLOTS * CS_TICKET_SLOT_WORDS * sizeof(unsigned)));
  HIP_TRY(hipMemset(m->d_tickets, 0, (size_t)CS_TICKET_SLOTS * CS_TICKET_SLOT_WORDS * sizeof(unsigned)));
  m->ticket_slots = CS_TICKET_SLOTS;
  m->shave_static = getenv("CSGPU_SHAVE_STATIC") != NULL; /* measurement switch: static shares instead of tickets */
  return CSGPU_OK;
}

/* several nodes per wave: kernel 5 and its 16-bit table relative to the pushing variable, cs_step_packed and
 * cs_step_import */
static int plan_packed(csgpu_model *m) {
  const cs_model *h = m->host;
  if (m->plan.shave.fn == NULL) return CSGPU_OK;
  const int n = h->n_vars, s3 = m->img->dense_slots == 3;
  m->packed_nw = 1; /* one set word per variable when every root domain has at most 32 values */
  for (int32_t v = 0; v < n; v++)
    if ((int64_t)h->dom[v].hi - (int64_t)h->dom[v].lo + 1 > 32) m->packed_nw = 2;
  m->packed_bias = 0;
  for (int32_t v = 0; v < n; v++)
    if (h->dom[v].lo - m->img->dense_dmin > m->packed_bias) m->packed_bias = h->dom[v].lo - m->img->dense_dmin;
  m->plan.packed_nodes = packed_nodes_per_wave(m->fb_words, n, m->img->dense_width);
  if (!m->plan.packed_nodes) return CSGPU_OK;
  const size_t bytes = m->dense_bytes;
  int rc;
  if ((rc = plan_kernel(&m->plan.packed, ne_packed_kernel(n, m->packed_nw, s3), 2 * bytes, m->plan.regs[0].waves))) return rc;
  m->plan.packed.per_cu = m->plan.regs[0].per_cu; /* its grid is kernel 4's */
  /* entry e of row u becomes e - (root_lo[u] - dmin) + bias (cs_kernels.hip.h, kernel 5) */
  const size_t per_row = (size_t)m->img->dense_slots * m->img->dense_cols, total = (size_t)n * per_row;
  uint16_t *rel = (uint16_t *)malloc(total * sizeof(uint16_t));
  const uint8_t *src = (const uint8_t *)m->img->dense_tab;
  for (size_t i = 0; i < total; i++) {
    const int32_t u = (int32_t)(i / per_row);
    rel[i] = src[i] == 0xffu ? (uint16_t)0xffffu : (uint16_t)((int)src[i] - (h->dom[u].lo - m->img->dense_dmin) + m->packed_bias);
  }
  rc = upload(rel, total * sizeof(uint16_t), (int **)&m->d_packed_tab);
  free(rel);
  if (rc) return rc;
  /* the step kernels: two workgroups of sixteen waves per CU */
  if (step_packed_lds(m, 16) <= 80u * 1024u &&
      ((rc = plan_kernel(&m->plan.step_packed, step_packed_kernel(n, m->packed_nw, s3), step_packed_lds(m, 16), 16)) ||
       (rc = plan_kernel(&m->plan.step_import, step_import_kernel(n, m->packed_nw, s3), (2 * bytes + 15) & ~(size_t)15, 4))))
    return rc;
  /* one word takes about 88 atomics per microsecond (MI355X_MICROARCH.md): with 32 parents per ticket a queens-16 frontier
   * of three million parents drew 78 tickets per microsecond and the whole launch waited for them (61 ms per search; 51 ms
   * with 64 and with 128 per ticket, 181 ms with 8) */
  m->step_chunk_max = 128;
  { const char *e = getenv("CSGPU_STEP_CHUNK_MAX"); if (e != NULL && atoi(e) > 0) m->step_chunk_max = atoi(e); } /* tuning */
  return CSGPU_OK;
}

/* the device and the mapped staging area of the single-node calls */
static int stage_single_node(csgpu_model *m) {
  int dev = 0;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  m->n_cus = prop.multiProcessorCount;
  const size_t nbytes = (size_t)(m->host->n_vars ? m->host->n_vars : 1) * sizeof(cs_val);
  const size_t part = (nbytes + 63) & ~(size_t)63;
  unsigned char *d = NULL;
  HIP_TRY(hipHostMalloc((void **)&m->h_one, 2 * part + 128, hipHostMallocMapped));
  HIP_TRY(hipHostGetDevicePointer((void **)&d, m->h_one, 0));
  m->d_one_in = (cs_val *)d;
  m->d_one_node = (cs_node_in *)(d + part);
  m->d_one_res = (cs_node_out *)(d + part + 64);
  m->d_one_out = (cs_val *)(d + part + 128);
  return CSGPU_OK;
}

extern "C" int csgpu_model_finalize(csgpu_model *m) {
  if (m == NULL) return set_err(CSGPU_E_ARG, "null argument");
  free_device(m);
  int rc;
  if ((rc = csgpu_model_build_tables(m)) || (rc = drop_entailed_clauses(m)) || (rc = plan_general(m)) ||
      (rc = plan_lds_resident(m)) || (rc = plan_forbidden_sets(m)) || (rc = plan_dense_table(m)) || (rc = plan_packed(m)) ||
      (rc = stage_single_node(m)))
    return rc;
  /* the search engine's step kernel: several nodes per wave, else cs_step_shave for intervals of at most 256 values */
  m->plan.step_kind = m->plan.step_packed.fn != NULL ? 1
                      : (m->plan.step_shave.fn != NULL && m->host->n_vars <= 256 && m->plan.max_width <= 256 ? 2 : 0);
  m->finalized = 1;
  return CSGPU_OK;
}

/* may the finalized model run kernel `which` (1-7)?  The one statement of the rules: what finalize planned */
static int kernel_qualifies(const csgpu_model *m, int which) {
  if (!m->finalized) return 0;
  switch (which) {
  case 1: return 1;
  case 2: return m->plan.lds.fn != NULL;
  case 3: return m->plan.bitset.fn != NULL;
  case 4: return m->plan.regs[0].fn != NULL;
  case 5: return m->plan.packed.fn != NULL;
  case 6: return m->plan.rounds.fn != NULL;
  case 7: return m->plan.shave.fn != NULL;
  default: return 0;
  }
}

extern "C" int csgpu_model_set_kernel(csgpu_model *m, int which) {
  static const char *const kernel_name[8] = {
    NULL, NULL, "the LDS-resident kernel", "the forbidden-set kernel", "the register-resident forbidden-set kernel",
    "the several-nodes-per-wave kernel (at most 32 variables, 64 values)", "the clause-resident kernel (at most 512 clauses)",
    "the interval-only shaving kernel (dense pair table in LDS)" };
  if (m == NULL || which < 0 || which > 7) return set_err(CSGPU_E_ARG, "bad argument");
  if (which >= 2) {
    if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
    if (!kernel_qualifies(m, which)) return set_err(CSGPU_E_LIMIT, "model does not qualify for %s", kernel_name[which]);
  }
  m->kernel_choice = which;
  return CSGPU_OK;
}

extern "C" int csgpu_model_qualifies(const csgpu_model *m, int which) { return m != NULL && kernel_qualifies(m, which); }

/* the planned instantiation of `family` (the order of cs_internal.h) by its dynamic symbol: the mangled name of the
 * very pointer the launchers use, "" when the family is not planned for this model */
extern "C" int csgpu_internal_plan_symbol(const csgpu_model *m, int family, char *buf, size_t len) {
  if (m == NULL || buf == NULL || len == 0) return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  const cs_kernel_plan *p = &m->plan;
  const cs_planned *fam[] = { &p->events, &p->traced, &p->rounds, &p->lds, &p->bitset, &p->regs[0], &p->regs[1],
                              &p->regs[2], &p->regs[3], &p->packed, &p->shave, &p->shave_trace, &p->server,
                              &p->step_shave, &p->step_packed, &p->step_import };
  if (family < 0 || family >= (int)(sizeof fam / sizeof fam[0])) return set_err(CSGPU_E_ARG, "no plan family %d", family);
  buf[0] = '\0';
  const void *fn = fam[family]->fn;
  if (fn == NULL) return CSGPU_OK;
  Dl_info info;
  if (dladdr(fn, &info) == 0 || info.dli_sname == NULL || info.dli_saddr != fn)
    return set_err(CSGPU_E_STATE, "plan family %d: the kernel handle has no dynamic symbol", family);
  if (strlen(info.dli_sname) >= len) return set_err(CSGPU_E_LIMIT, "plan family %d: symbol longer than the buffer", family);
  strcpy(buf, info.dli_sname);
  return CSGPU_OK;
}

/* the same for the cs_dive_* and the cs_walk_* kernels, which are no families of the list above (the plan dictionary
 * stays what it was): the instantiation of `k`, a kernel called `name`, by its dynamic symbol ("" where the model plans
 * none; k is NULL with m) */
static int many_symbol(const csgpu_model *m, const cs_planned *k, const char *name, char *buf, size_t len) {
  if (m == NULL || buf == NULL || len == 0) return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  buf[0] = '\0';
  const void *fn = k->fn;
  if (fn == NULL) return CSGPU_OK;
  Dl_info info;
  if (dladdr(fn, &info) == 0 || info.dli_sname == NULL || info.dli_saddr != fn)
    return set_err(CSGPU_E_STATE, "%s: the kernel handle has no dynamic symbol", name);
  if (strlen(info.dli_sname) >= len) return set_err(CSGPU_E_LIMIT, "%s: symbol longer than the buffer", name);
  strcpy(buf, info.dli_sname);
  return CSGPU_OK;
}

#define MANY_SYMBOL(EXPORT, PLANNED, NAMES, FAMILY)                                       \
  extern "C" int EXPORT(const csgpu_model *m, char *buf, size_t len) {                    \
    return many_symbol(m, m != NULL ? &m->plan.PLANNED[FAMILY] : NULL, NAMES[FAMILY], buf, len); \
  }
MANY_SYMBOL(csgpu_internal_many_symbol, dive, many_kernel_name, MANY_PLAIN)
MANY_SYMBOL(csgpu_internal_many_resume_symbol, dive, many_kernel_name, MANY_CK)
MANY_SYMBOL(csgpu_internal_many_upto_symbol, dive, many_kernel_name, MANY_UPTO)
MANY_SYMBOL(csgpu_internal_many_restart_symbol, dive, many_kernel_name, MANY_RESTART)
MANY_SYMBOL(csgpu_internal_many_stream_symbol, dive, many_kernel_name, MANY_STREAM)
MANY_SYMBOL(csgpu_internal_many_allowed_symbol, dive, many_kernel_name, MANY_ALLOWED)
MANY_SYMBOL(csgpu_internal_many_allowed_upto_symbol, dive, many_kernel_name, MANY_ALLOWED_UPTO)
MANY_SYMBOL(csgpu_internal_many_allowed_resume_symbol, dive, many_kernel_name, MANY_ALLOWED_CK)
MANY_SYMBOL(csgpu_internal_many_allowed_upto_resume_symbol, dive, many_kernel_name, MANY_ALLOWED_UPTO_CK)
MANY_SYMBOL(csgpu_internal_many_clauses_symbol, walk, walk_kernel_name, WALK_PLAIN)
MANY_SYMBOL(csgpu_internal_many_clauses_resume_symbol, walk, walk_kernel_name, WALK_CK)
MANY_SYMBOL(csgpu_internal_many_clauses_upto_symbol, walk, walk_kernel_name, WALK_UPTO)
MANY_SYMBOL(csgpu_internal_many_clauses_restart_symbol, walk, walk_kernel_name, WALK_RESTART)
MANY_SYMBOL(csgpu_internal_many_clauses_stream_symbol, walk, walk_kernel_name, WALK_STREAM)
MANY_SYMBOL(csgpu_internal_many_clauses_from_symbol, walk, walk_kernel_name, WALK_FROM)
MANY_SYMBOL(csgpu_internal_many_clauses_order_symbol, walk, walk_kernel_name, WALK_ORDER)
MANY_SYMBOL(csgpu_internal_many_clauses_order_resume_symbol, walk, walk_kernel_name, WALK_ORDER_CK)
MANY_SYMBOL(csgpu_internal_many_clauses_order_from_symbol, walk, walk_kernel_name, WALK_ORDER_FROM)
MANY_SYMBOL(csgpu_internal_many_clauses_wide_symbol, walk, walk_kernel_name, WALK_WIDE)
MANY_SYMBOL(csgpu_internal_many_clauses_wide_resume_symbol, walk, walk_kernel_name, WALK_WIDE_CK)
#undef MANY_SYMBOL

extern "C" void csgpu_internal_engine_ref(const csgpu_model *m, int delta) {
  if (m != NULL) const_cast<csgpu_model *>(m)->engines += delta;
}

extern "C" const int32_t *csgpu_internal_root_lo(const csgpu_model *m) {
  return m != NULL && m->finalized && m->fb_words ? m->d_root_lo : NULL;
}

extern "C" int csgpu_model_forbidden_words(const csgpu_model *m) { return m && m->finalized ? m->fb_words : 0; }

extern "C" int csgpu_internal_step_kind(const csgpu_model *m) { return m == NULL || !m->finalized ? 0 : m->plan.step_kind; }

/* waves of a cs_step_shave launch with `stage_rows` staging rows: the resident grid, fewer when a wave's region would
 * not hold the children of four parents */
static int64_t step_shave_waves(const csgpu_model *m, int64_t stage_rows) {
  const cs_planned *k = &m->plan.step_shave;
  int64_t waves = (int64_t)m->n_cus * (int64_t)k->per_cu * k->waves;
  const int64_t by_stage = stage_rows / (4 * (int64_t)m->plan.max_width);
  if (waves > by_stage) waves = by_stage / k->waves * k->waves;
  return waves;
}

extern "C" int64_t csgpu_internal_step_parents_limit(const csgpu_model *m, int64_t stage_rows) {
  const int kind = csgpu_internal_step_kind(m);
  if (kind == 1) return 0x3fffffff;
  if (kind != 2) return 0;
  const int maxw = m->plan.max_width;
  const int64_t waves = step_shave_waves(m, stage_rows);
  if (waves < 1) return 0;
  return (stage_rows - waves * 2 * maxw) / maxw; /* every child of every parent may survive, and a wave stops two parents short of its region's end */
}

extern "C" int64_t csgpu_internal_step_stage_rows(const csgpu_model *m) {
  if (csgpu_internal_step_kind(m) != 2) return 0;
  return (int64_t)m->n_cus * 32 * 4 * m->plan.max_width;
}

extern "C" int64_t csgpu_internal_step_waves(const csgpu_model *m) { return m == NULL ? 0 : (int64_t)m->n_cus * 32; }

static int launch_step_shave(const csgpu_model *m, const csgpu_step_launch *L, void *stream) {
  const cs_planned *k = &m->plan.step_shave;
  const int n = m->host->n_vars, maxw = m->plan.max_width;
  int64_t waves = step_shave_waves(m, L->stage_rows);
  if (waves < k->waves || (int64_t)L->parents > csgpu_internal_step_parents_limit(m, L->stage_rows))
    return set_err(CSGPU_E_LIMIT, "step kernel: staging buffer too small for the frontier");
  const int64_t by_parents = ((int64_t)L->parents + k->waves - 1) / k->waves * k->waves;
  if (waves > by_parents) waves = by_parents;
  const int64_t grid = waves / k->waves;
  const int64_t K = L->stage_rows / waves;
  cs_step_io io;
  io.pool = (const uint2 *)L->pool;
  io.first_row = (long long)L->first_row;
  io.parents = L->parents;
  io.chunk = 1;
  io.maxw = maxw;
  io.stage = (uint2 *)L->stage;
  io.K = (int)(K > 0x7fffffff ? 0x7fffffff : K);
  io.fill = L->fill;
  io.wstat = (unsigned long long *)L->wstat;
  io.ticket = L->ticket;
  io.solutions = L->solutions;
  io.stored = (unsigned long long *)L->stored;
  io.max_solutions = (long long)L->max_solutions;
  io.store_open = L->store_open;
  io.stream_on = L->stream != NULL;
  int nn = n, slots = m->img->dense_slots, dmin_d = m->img->dense_dmin;
  const void *tab_d = m->d_dense_tab;
  const int *root_lo_d = m->d_root_lo, *sym_off = m->d_sym_off;
  size_t tab_bytes = m->dense_bytes;
  void *args[] = { &nn, &tab_d, &slots, &dmin_d, &root_lo_d, &sym_off, &tab_bytes, &io };
  HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)grid), dim3((unsigned)(k->waves * CS_WAVE)), args, k->lds, (hipStream_t)stream));
  hipLaunchKernelGGL(cs_collect, dim3((unsigned)waves), dim3(256), 0, (hipStream_t)stream, (const unsigned *)L->fill, (int)waves,
                     (const uint2 *)L->stage, io.K, n, (uint2 *)L->pool, (long long)L->first_row, (int)L->parents,
                     0 /* every parent is drawn */, (const unsigned *)L->ticket, (const unsigned long long *)L->wstat,
                     (unsigned long long *)L->out, (const unsigned long long *)L->stored,
                     L->stream, (long long)L->stream_base, (long long)L->stream_limit, (long long)L->stream_cap,
                     (unsigned long long *)L->stream_err);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_internal_step(const csgpu_model *m, const csgpu_step_launch *L, void *stream) {
  const int kind = csgpu_internal_step_kind(m);
  if (kind == 0 || L == NULL || L->parents < 1) return set_err(CSGPU_E_ARG, "bad argument");
  if (kind == 2) return launch_step_shave(m, L, stream);
  const int n = m->host->n_vars;
  const int G = m->plan.packed_nodes, maxw = m->plan.max_width;
  if (G * maxw > CS_STEP_QN) return set_err(CSGPU_E_LIMIT, "step kernel: interval too wide for the child queue");
  /* waves: the machine's, fewer when the staging buffer would leave a wave less than two rounds of worst-case children;
   * and no more than the parents need */
  int64_t waves = (int64_t)m->n_cus * 32;
  const int64_t by_stage = L->stage_rows / (2 * (int64_t)G * maxw);
  if (waves > by_stage) waves = by_stage;
  const int64_t by_parents = ((int64_t)L->parents + G - 1) / G;
  if (waves > by_parents) waves = by_parents;
  if (waves < 1) return set_err(CSGPU_E_LIMIT, "step kernel: staging buffer too small");
  int wg_waves = 16;
  while (wg_waves > waves) wg_waves >>= 1;
  const int64_t grid = waves / wg_waves;
  waves = grid * wg_waves;
  const int64_t K = L->stage_rows / waves;
  /* parents per ticket: about eight tickets per wave, at most step_chunk_max, and a chunk's worst case fits half a region */
  int64_t chunk = (int64_t)L->parents / (waves * 8);
  if (chunk > m->step_chunk_max) chunk = m->step_chunk_max;
  if (chunk * maxw > K / 2) chunk = K / (2 * maxw);
  chunk = chunk / G * G;
  if (chunk < G) chunk = G;
  cs_step_io io;
  io.pool = (const uint2 *)L->pool;
  io.first_row = (long long)L->first_row;
  io.parents = L->parents;
  io.chunk = (int)chunk;
  io.maxw = maxw;
  io.stage = (uint2 *)L->stage;
  io.K = (int)(K > 0x7fffffff ? 0x7fffffff : K);
  io.fill = L->fill;
  io.wstat = (unsigned long long *)L->wstat;
  io.ticket = L->ticket;
  io.solutions = L->solutions;
  io.stored = (unsigned long long *)L->stored;
  io.max_solutions = (long long)L->max_solutions;
  io.store_open = L->store_open;
  io.stream_on = L->stream != NULL;
  int nn = n, slots = m->img->dense_slots, bias = m->packed_bias;
  const void *tab_d = m->d_packed_tab;
  const int *root_lo_d = m->d_root_lo, *sym_off = m->d_sym_off;
  size_t tab_bytes = 2 * m->dense_bytes;
  void *args[] = { &nn, &tab_d, &slots, &root_lo_d, &sym_off, &bias, &tab_bytes, &io };
  HIP_TRY(hipLaunchKernel(m->plan.step_packed.fn, dim3((unsigned)grid), dim3((unsigned)(wg_waves * CS_WAVE)), args,
                          step_packed_lds(m, wg_waves), (hipStream_t)stream));
  hipLaunchKernelGGL(cs_collect, dim3((unsigned)waves), dim3(256), 0, (hipStream_t)stream, (const unsigned *)L->fill, (int)waves,
                     (const uint2 *)L->stage, io.K, n, (uint2 *)L->pool, (long long)L->first_row, (int)L->parents,
                     (int)chunk, (const unsigned *)L->ticket, (const unsigned long long *)L->wstat,
                     (unsigned long long *)L->out, (const unsigned long long *)L->stored,
                     L->stream, (long long)L->stream_base, (long long)L->stream_limit, (long long)L->stream_cap,
                     (unsigned long long *)L->stream_err);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_internal_step_import(const csgpu_model *m, csgpu_val *d_rows, int64_t first_row, int64_t count,
                                          void *stream) {
  const int kind = csgpu_internal_step_kind(m);
  if (kind == 2) return CSGPU_OK; /* that path's pool holds interval rows */
  if (kind != 1 || d_rows == NULL || count < 0) return set_err(CSGPU_E_ARG, "bad argument");
  if (count == 0) return CSGPU_OK;
  const cs_planned *k = &m->plan.step_import;
  const int n = m->host->n_vars, G = m->plan.packed_nodes;
  int nn = n, slots = m->img->dense_slots, bias = m->packed_bias;
  const void *tab_d = m->d_packed_tab;
  const int *root_lo_d = m->d_root_lo;
  size_t tab_bytes = 2 * m->dense_bytes;
  long long fr = first_row, cnt = count;
  int64_t grid = (count + (int64_t)G * k->waves - 1) / ((int64_t)G * k->waves); /* G rows per wave and step */
  if (grid > (int64_t)m->n_cus * 8) grid = (int64_t)m->n_cus * 8;
  void *args[] = { &nn, &tab_d, &slots, &root_lo_d, &bias, &tab_bytes, &d_rows, &fr, &cnt };
  HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)grid), dim3((unsigned)(k->waves * CS_WAVE)), args, k->lds, (hipStream_t)stream));
  return CSGPU_OK;
}

extern "C" int csgpu_internal_step_export(const csgpu_model *m, csgpu_val *d_rows, int64_t first_row, int64_t count,
                                          void *stream) {
  const int kind = csgpu_internal_step_kind(m);
  if (kind == 2) return CSGPU_OK;
  if (kind != 1 || d_rows == NULL || count < 0) return set_err(CSGPU_E_ARG, "bad argument");
  if (count == 0) return CSGPU_OK;
  const int n = m->host->n_vars;
  const long long elements = (long long)count * n;
  uint2 *rows = (uint2 *)d_rows + (size_t)first_row * n;
  const unsigned grid = (unsigned)((elements + 255) / 256);
  if (m->packed_nw == 1)
    hipLaunchKernelGGL(cs_step_export<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, (const int *)m->d_root_lo, rows, elements);
  else
    hipLaunchKernelGGL(cs_step_export<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, (const int *)m->d_root_lo, rows, elements);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

/* the register-resident forbidden-set kernel (kernel 4); sets_only: the states are the sets alone */
static int launch_regs(const csgpu_model *m, const csgpu_val *d_states_in, const uint64_t *d_forb_in,
                       const csgpu_node *d_nodes, csgpu_val *d_states_out, uint64_t *d_forb_out, csgpu_result *d_results,
                       int64_t batch, const uint64_t *d_batch, int sets_only, int flags, void *stream) {
  int csz = shrink_chunk(CS_CHUNK, batch, (int64_t)m->n_cus * 32);
  int n = m->host->n_vars, slots = m->img->dense_slots, dmin_d = m->img->dense_dmin;
  const void *tab_d = m->d_dense_tab;
  const int *root_lo_d = m->d_root_lo, *sym_off = m->d_sym_off;
  long long nb_d = (long long)batch;
  void *args_d[] = { &n, &tab_d, &slots, &dmin_d, &root_lo_d, &sym_off, &d_states_in, &d_forb_in, &d_nodes,
                     &d_states_out, &d_forb_out, &d_results, &nb_d, &d_batch, &csz, &flags };
  if (!sets_only && m->kernel_choice != 4 && kernel_qualifies(m, 5)) { /* kernel 5: one wave per group of nodes, grid-stride */
    const cs_planned *k = &m->plan.packed;
    const int64_t groups = (batch + m->plan.packed_nodes - 1) / m->plan.packed_nodes;
    int64_t gp = (int64_t)m->n_cus * (int64_t)k->per_cu * 2;
    const int64_t need_gp = (groups + k->waves - 1) / k->waves;
    if (gp > need_gp) gp = need_gp;
    csz = m->packed_bias; /* this kernel's arguments in those positions */
    tab_d = m->d_packed_tab;
    HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)gp), dim3((unsigned)(k->waves * CS_WAVE)), args_d, k->lds, (hipStream_t)stream));
    return CSGPU_OK;
  }
  const int fast = m->plan.full && d_forb_in != NULL && d_forb_out != NULL && flags == 0;
  const cs_planned *k = &m->plan.regs[fast | sets_only << 1];
  const int64_t chunks = (batch + csz - 1) / csz;
  int64_t g = (int64_t)m->n_cus * (int64_t)k->per_cu;
  const int64_t need_wg = (chunks + k->waves - 1) / k->waves;
  g *= 2; /* twice the resident grid: the dispatcher backfills CUs whose waves finish early (measured +1.5 %) */
  if (g > need_wg) g = need_wg;
  HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)g), dim3((unsigned)(k->waves * CS_WAVE)), args_d, k->lds, (hipStream_t)stream));
  return CSGPU_OK;
}

/* kernel 7: intervals in, intervals out */
static std::mutex g_ticket_mutex;

/* the ticket slot of a launch on `stream` (NULL: none left, the kernel then uses static shares) */
static unsigned *ticket_slot(csgpu_model *m, void *stream) {
  if (m->d_tickets == NULL) return NULL;
  std::lock_guard<std::mutex> lock(g_ticket_mutex);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (stream != NULL && hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
  int slot = -1;
  if (cap == hipStreamCaptureStatusActive) {
    /* a captured launch keeps a slot of its own for good (taken from the top) */
    if (m->ticket_reserved < m->ticket_slots - CS_TICKET_STREAMS) slot = m->ticket_slots - 1 - m->ticket_reserved++;
  } else {
    for (int i = 0; i < m->ticket_streams; i++)
      if (m->ticket_stream[i] == stream) slot = i;
    if (slot < 0 && m->ticket_streams < CS_TICKET_STREAMS) {
      slot = m->ticket_streams++;
      m->ticket_stream[slot] = stream;
    }
  }
  return slot < 0 ? NULL : m->d_tickets + (size_t)slot * CS_TICKET_SLOT_WORDS;
}

/* the geometry of a kernel 7 launch of `batch` nodes: nodes per chunk, and the grid in workgroups of plan.shave.waves */
static void shave_geometry(const csgpu_model *m, int64_t batch, int *csz_out, int64_t *grid_out) {
  const cs_planned *k = &m->plan.shave;
  /* four or two nodes per chunk (four per ticket when a node is one register per lane); fewer while that would leave a
   * wave with less than four chunks */
  const int csz = shrink_chunk(m->host->n_vars <= CS_WAVE ? 2 * CS_SHAVE_CHUNK : CS_SHAVE_CHUNK, batch, 4 * (int64_t)m->n_cus * 32);
  const int64_t chunks = (batch + csz - 1) / csz;
  int64_t g = (int64_t)m->n_cus * (int64_t)k->per_cu; /* the resident grid: persistent waves, work drawn by ticket */
  const int64_t need_wg = (chunks + k->waves - 1) / k->waves;
  if (g > need_wg) g = need_wg;
  *csz_out = csz;
  *grid_out = g;
}

extern "C" int csgpu_internal_shave_launch(const csgpu_model *m, int64_t batch, int64_t out[3]) {
  if (m == NULL || out == NULL || batch < 1) return set_err(CSGPU_E_ARG, "bad argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (!kernel_qualifies(m, 7)) return set_err(CSGPU_E_LIMIT, "model does not qualify for the interval-only shaving kernel");
  int csz;
  int64_t g;
  shave_geometry(m, batch, &csz, &g);
  out[0] = g;
  out[1] = m->plan.shave.waves;
  out[2] = csz;
  return CSGPU_OK;
}

static int launch_shave(const csgpu_model *m, const csgpu_val *d_states_in, const csgpu_node *d_nodes,
                        csgpu_val *d_states_out, csgpu_result *d_results, int64_t batch, const uint64_t *d_batch,
                        void *stream) {
  const cs_planned *k = &m->plan.shave;
  int csz;
  int64_t g;
  shave_geometry(m, batch, &csz, &g);
  int n = m->host->n_vars, slots = m->img->dense_slots, dmin_d = m->img->dense_dmin;
  const void *tab_d = m->d_dense_tab;
  const int *root_lo_d = m->d_root_lo, *sym_off = m->d_sym_off;
  long long nb_d = (long long)batch;
  unsigned *tickets = m->shave_static ? NULL : ticket_slot((csgpu_model *)m, stream);
  int4 *no_trace = NULL;
  unsigned *no_trace_n = NULL;
  unsigned no_trace_cap = 0u;
  void *args[] = { &n, &tab_d, &slots, &dmin_d, &root_lo_d, &sym_off, &d_states_in, &d_nodes, &d_states_out, &d_results,
                   &nb_d, &d_batch, &csz, &tickets, &no_trace, &no_trace_n, &no_trace_cap };
  HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)g), dim3((unsigned)(k->waves * CS_WAVE)), args, k->lds, (hipStream_t)stream));
  return CSGPU_OK;
}

/* ---- the csgpu_solve_many family: a depth-first search per wavefront (cs_dive.hip.h) ---- */

static_assert(sizeof(csgpu_many_result) == sizeof(cs_dive_result) && sizeof(csgpu_many_result) == 40, "csgpu_many_result layout");
static_assert(sizeof(csgpu_many_restart_options) == 24, "csgpu_many_restart_options layout");

#define MANY_NOT_QUALIFIED "model does not qualify for the interval-only shaving kernel"

struct csgpu_many_checkpoints {
  const csgpu_model *m;
  int64_t capacity;
  size_t slot_bytes;
  cs_val *d_pool;
  unsigned long long *d_next; /* slots handed out since the last reset */
  int counted;                /* the model counts this pool among the objects that hold its device tables */
  int kind;                   /* MANY_POOL_DIVE: of csgpu_many_checkpoints_create; MANY_POOL_WALK: of the clause one;
                                 MANY_POOL_ORDER: of csgpu_many_clause_ordered_checkpoints_create; MANY_POOL_WIDE: of
                                 csgpu_many_clause_wide_checkpoints_create */
  int *d_zero;                /* the clause kinds: n_vars zeros, the offsets cs_dive_export adds to absolute bounds */
  int frames;                 /* the frames a slot has for a stack: n_vars, MANY_POOL_ORDER: csgpu_many_clauses_ordered_frames */
  int split_width;            /* MANY_POOL_ORDER: the split_width the pool was made for (never 0: 256 stands there) */
};
enum { MANY_POOL_DIVE, MANY_POOL_WALK, MANY_POOL_ORDER, MANY_POOL_WIDE };
#define MANY_POOL_KIND "the checkpoint pool is of the other kind: csgpu_many_checkpoints_create makes the pools of csgpu_solve_many, " \
                       "csgpu_many_clause_checkpoints_create those of csgpu_solve_many_clauses"
#define MANY_POOL_KIND_ORDER "the checkpoint pool is of the other kind: csgpu_many_clause_ordered_checkpoints_create makes the pools of " \
                             "csgpu_solve_many_clauses_ordered_checkpointed / _resume, and only those"
#define MANY_POOL_KIND_WIDE "the checkpoint pool is of the other kind: csgpu_many_clause_wide_checkpoints_create makes the pools of " \
                            "csgpu_solve_many_clauses_wide_checkpointed / _wide_resume, and only those"

extern "C" int64_t csgpu_internal_many_waves(const csgpu_model *m, int64_t count) {
  if (m == NULL || !m->finalized || m->plan.dive[MANY_PLAIN].fn == NULL || count < 1) return 0;
  const cs_planned *k = &m->plan.dive[MANY_PLAIN]; /* the five are planned alike */
  int64_t grid = (int64_t)m->n_cus * k->per_cu;
  const int64_t by_count = (count + k->waves - 1) / k->waves;
  if (grid > by_count) grid = by_count;
  return grid * k->waves;
}

/* the model's ticket counters and, for `waves` > 0, stacks of `frames` frames for that many waves.  The block is the
 * whole family's and the families differ in their frames per wave: it grows by its bytes, not by its waves */
static int many_workspace(csgpu_model *mm, int64_t waves, int frames) {
  const int n = mm->host->n_vars;
  const size_t bytes = (size_t)waves * (size_t)frames * ((size_t)n + 1) * sizeof(cs_val);
  if (mm->d_many_tickets == NULL) {
    quiesce_servers();
    HIP_TRY(hipMalloc((void **)&mm->d_many_tickets, (size_t)CS_DIVE_SHARDS * CS_DIVE_TICKET_STRIDE * sizeof(unsigned)));
    HIP_TRY(hipMemset(mm->d_many_tickets, 0, (size_t)CS_DIVE_SHARDS * CS_DIVE_TICKET_STRIDE * sizeof(unsigned)));
  }
  if (mm->many_stack_bytes < bytes) { /* one call in flight per model: nothing reads the old workspace */
    quiesce_servers();
    if (mm->d_many_stack != NULL) (void)hipFree(mm->d_many_stack);
    mm->d_many_stack = NULL;
    mm->many_stack_bytes = 0;
    HIP_TRY(hipMalloc(&mm->d_many_stack, bytes));
    mm->many_stack_bytes = bytes;
  }
  return CSGPU_OK;
}

/* The checks of every entry point, none of which touches the device: many_check_head, then the call's own checks of its
 * options, then many_check_tail.  `null_arg`: some required pointer is NULL (max_nodes is then not looked at). */
static int many_check_head(int null_arg, int64_t count, int64_t max_nodes, const char *budgeted) {
  if (null_arg) return set_err(CSGPU_E_ARG, "null argument");
  if (count < 0) return set_err(CSGPU_E_ARG, "negative instance count");
  if (max_nodes <= 0) return set_err(CSGPU_E_ARG, "max_nodes must be positive: every %s has a budget", budgeted);
  return CSGPU_OK;
}

static int many_check_objective(int objective) {
  if (objective == CS_OBJ_MIN || objective == CS_OBJ_MAX)
    return set_err(CSGPU_E_LIMIT, "csgpu_solve_many searches with ANY or ALL: MIN / MAX are not supported");
  if (objective != CS_OBJ_ANY && objective != CS_OBJ_ALL) return set_err(CSGPU_E_ARG, "no objective %d", objective);
  return CSGPU_OK;
}

/* `ck`: the pool of a call that has one, else NULL */
static int many_check_tail(const csgpu_model *m, int family, const csgpu_many_checkpoints *ck, int64_t count) {
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (m->plan.dive[family].fn == NULL)
    return set_err(CSGPU_E_LIMIT, MANY_NOT_QUALIFIED " (a pure != network of at most 256 variables whose dense pair table "
                                                     "fits LDS), which csgpu_solve_many is built on");
  if (ck != NULL && ck->m != m) return set_err(CSGPU_E_ARG, "the checkpoint pool was created for another model");
  if (ck != NULL && ck->kind != MANY_POOL_DIVE) return set_err(CSGPU_E_ARG, MANY_POOL_KIND);
  if (count > 0x7fffffff - CS_DIVE_SHARDS) return set_err(CSGPU_E_LIMIT, "more than 2^31 - 65 instances in one call");
  return CSGPU_OK;
}

/* The one launch of a cs_dive_* kernel, after the checks.  `tail0`, `tail1`: the family's own kernel arguments after the
 * nine common ones (NULL where it has fewer).  `resume`: the instances go on in the frames of their checkpoint slots, so
 * the call brings no roots and needs no stacks. */
static int many_launch(const csgpu_model *m, int family, const csgpu_val *d_roots, int64_t count, int64_t max_nodes, int all,
                       csgpu_many_result *d_results, int32_t *d_solutions, int resume, void *stream, void *tail0, void *tail1) {
  if (count == 0) return CSGPU_OK;
  csgpu_model *mm = const_cast<csgpu_model *>(m);
  const cs_planned *k = &m->plan.dive[family];
  const int n = m->host->n_vars;
  const int64_t waves = csgpu_internal_many_waves(m, count);
  const int frames = n; /* open levels + 1: at most n - 1 frames are in use, the n-th keeps the root node's fixpoint */
  int rc;
  if ((rc = many_workspace(mm, resume ? 0 : waves, frames))) return rc;
  cs_dive_io io;
  io.roots = (const cs_val *)d_roots;
  io.count = (int)count;
  io.all = all;
  io.max_nodes = (long long)max_nodes;
  io.results = (cs_dive_result *)d_results;
  io.solutions = d_solutions;
  io.stack = resume ? NULL : (cs_val *)mm->d_many_stack;
  io.frames = frames;
  io.tickets = mm->d_many_tickets;
  int nn = n, slots = m->img->dense_slots, dmin_d = m->img->dense_dmin;
  const void *tab_d = m->d_dense_tab;
  const int *root_lo_d = m->d_root_lo, *root_hi_d = m->d_root_hi, *sym_off = m->d_sym_off;
  size_t tab_bytes = m->dense_bytes;
  void *args[] = { &nn, &tab_d, &slots, &dmin_d, &root_lo_d, &root_hi_d, &sym_off, &tab_bytes, &io, tail0, tail1 };
  HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)(waves / k->waves)), dim3((unsigned)(k->waves * CS_WAVE)), args, k->lds, (hipStream_t)stream));
  return CSGPU_OK;
}

/* the pool and slot numbers as the kernels take them; ck == NULL: a pool of capacity 0 that cs_dive_upto does not touch */
static cs_dive_ck many_ck_arg(const csgpu_many_checkpoints *ck, int32_t *d_slots, int resume) {
  cs_dive_ck dk;
  dk.pool = ck != NULL ? ck->d_pool : NULL;
  dk.next = ck != NULL ? ck->d_next : NULL;
  dk.capacity = ck != NULL ? (int)ck->capacity : 0;
  dk.resume = resume;
  dk.slots = ck != NULL ? d_slots : NULL;
  return dk;
}

extern "C" int csgpu_solve_many(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_options *options,
                                csgpu_many_result *d_results, int32_t *d_solutions, void *stream) {
  const int null_arg = m == NULL || d_roots == NULL || d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "instance")) ||
      (rc = many_check_objective(options->objective)) || (rc = many_check_tail(m, MANY_PLAIN, NULL, count)))
    return rc;
  return many_launch(m, MANY_PLAIN, d_roots, count, options->max_nodes, options->objective == CS_OBJ_ALL, d_results, d_solutions,
                     0, stream, NULL, NULL);
}

/* ---- checkpoints: csgpu_solve_many in slices (cs_dive_resume) ---- */

/* does the model run the cs_dive_* kernels?  What finalize planned; before finalize, the same rules on the host tables
 * (csgpu_model_build_tables), which is all they depend on */
static int many_qualifies(const csgpu_model *m) {
  if (m->finalized) return m->plan.dive[MANY_PLAIN].fn != NULL;
  if (m->img == NULL) return 0;
  int fw = 0;
  size_t bytes = 0;
  return forbidden_sets_shape(m, &fw, &bytes) > 0 && dense_table_waves(m, &bytes) > 0 && ((bytes + 15) & ~(size_t)15) <= CS_CU_LDS;
}

extern "C" size_t csgpu_many_checkpoint_bytes(const csgpu_model *m) {
  if (m == NULL || !many_qualifies(m)) return 0;
  const size_t n = (size_t)m->host->n_vars;
  return (n + 1) * (n + 1) * sizeof(cs_val); /* the header frame, n - 1 stack frames at most, the current node */
}

/* the pool of either kind, after the checks of its create call; `qualifies`: may the model's kernels of that kind run? */
static int many_pool_create(const csgpu_model *m, int64_t capacity, int kind, int qualifies, const char *limit, size_t slot_bytes,
                            int frames, int split_width, csgpu_many_checkpoints **out) {
  if (m == NULL || out == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (capacity < 1) return set_err(CSGPU_E_ARG, "a checkpoint pool has at least one slot");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (!qualifies) return set_err(CSGPU_E_LIMIT, "%s", limit);
  if (capacity > 0x7fffffff) return set_err(CSGPU_E_LIMIT, "more than 2^31 - 1 slots");
  csgpu_many_checkpoints *ck = (csgpu_many_checkpoints *)calloc(1, sizeof *ck);
  if (ck == NULL) return set_err(CSGPU_E_LIMIT, "out of memory");
  ck->m = m;
  ck->capacity = capacity;
  ck->slot_bytes = slot_bytes;
  ck->kind = kind;
  ck->frames = frames;
  ck->split_width = split_width;
  const size_t zero_bytes = (size_t)m->host->n_vars * sizeof(int);
  hipError_t e;
  if ((e = hipMalloc((void **)&ck->d_pool, (size_t)capacity * ck->slot_bytes)) != hipSuccess ||
      (e = hipMalloc((void **)&ck->d_next, sizeof *ck->d_next)) != hipSuccess ||
      (e = hipMemset(ck->d_pool, 0, (size_t)capacity * ck->slot_bytes)) != hipSuccess || /* no slot holds a checkpoint */
      (e = hipMemset(ck->d_next, 0, sizeof *ck->d_next)) != hipSuccess ||
      (kind != MANY_POOL_DIVE && ((e = hipMalloc((void **)&ck->d_zero, zero_bytes)) != hipSuccess ||
                                  (e = hipMemset(ck->d_zero, 0, zero_bytes)) != hipSuccess))) {
    csgpu_many_checkpoints_free(ck);
    return set_err(CSGPU_E_HIP, "checkpoint pool of %lld slots: %s", (long long)capacity, hipGetErrorString(e));
  }
  csgpu_internal_engine_ref(m, 1); /* the pool reads the model's device tables: no clause is added under it */
  ck->counted = 1;
  *out = ck;
  return CSGPU_OK;
}

extern "C" int csgpu_many_checkpoints_create(const csgpu_model *m, int64_t capacity, csgpu_many_checkpoints **out) {
  return many_pool_create(m, capacity, MANY_POOL_DIVE, m != NULL && m->finalized && m->plan.dive[MANY_CK].fn != NULL,
                          MANY_NOT_QUALIFIED ", which csgpu_solve_many is built on", csgpu_many_checkpoint_bytes(m),
                          m != NULL ? m->host->n_vars : 0, 0, out);
}

extern "C" int csgpu_many_checkpoints_reset(csgpu_many_checkpoints *ck, void *stream) {
  if (ck == NULL) return set_err(CSGPU_E_ARG, "null argument");
  HIP_TRY(hipMemsetAsync(ck->d_next, 0, sizeof *ck->d_next, (hipStream_t)stream));
  return CSGPU_OK;
}

extern "C" void csgpu_many_checkpoints_free(csgpu_many_checkpoints *ck) {
  if (ck == NULL) return;
  if (ck->counted) csgpu_internal_engine_ref(ck->m, -1);
  (void)hipFree(ck->d_pool);
  (void)hipFree(ck->d_next);
  (void)hipFree(ck->d_zero);
  free(ck);
}

/* csgpu_solve_many_checkpointed, and with `resume` (and no roots) csgpu_solve_many_resume */
static int many_ck_call(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_options *options,
                        csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots,
                        int resume, void *stream) {
  const int null_arg = m == NULL || (!resume && d_roots == NULL) || d_results == NULL || options == NULL || ck == NULL || d_slots == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "slice")) ||
      (rc = many_check_objective(options->objective)) || (rc = many_check_tail(m, MANY_CK, ck, count)))
    return rc;
  cs_dive_ck dk = many_ck_arg(ck, d_slots, resume);
  return many_launch(m, MANY_CK, d_roots, count, options->max_nodes, options->objective == CS_OBJ_ALL, d_results, d_solutions,
                     resume, stream, &dk, NULL);
}

extern "C" int csgpu_solve_many_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                             const csgpu_many_options *options, csgpu_many_result *d_results,
                                             int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream) {
  return many_ck_call(m, d_roots, count, options, d_results, d_solutions, ck, d_slots, 0, stream);
}

extern "C" int csgpu_solve_many_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options,
                                       csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck,
                                       int32_t *d_slots, void *stream) {
  return many_ck_call(m, NULL, count, options, d_results, d_solutions, ck, d_slots, 1, stream);
}

/* the open subtrees of a slot of any kind: `head`, if wanted, receives the header's first two entries.  A clause pool
 * holds absolute bounds: cs_dive_export adds the pool's zeros to them.  A slot has ck->frames + 1 frames, depth < ck->frames */
static int many_pool_states(const csgpu_many_checkpoints *ck, int kind, int32_t slot, csgpu_val *d_states, int64_t cap,
                            int64_t *count, cs_val *head2, void *stream) {
  if (ck == NULL || d_states == NULL || count == NULL || cap < 0) return set_err(CSGPU_E_ARG, "null argument");
  if (ck->kind != kind) return set_err(CSGPU_E_ARG, MANY_POOL_KIND);
  if (slot < 0 || slot >= ck->capacity) return set_err(CSGPU_E_ARG, "no slot %d in a pool of %lld", slot, (long long)ck->capacity);
  const int n = ck->m->host->n_vars;
  const cs_val *base = ck->d_pool + (size_t)slot * ((size_t)ck->frames + 1) * ((size_t)n + 1);
  cs_val header[2];
  HIP_TRY(hipMemcpyAsync(header, base, sizeof header, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  const cs_val head = header[0];
  const int magic_ok = kind == MANY_POOL_WALK    ? head.hi == CS_WALK_CK_MAGIC
                       : kind == MANY_POOL_ORDER ? head.hi == CS_WALK_CK_MAGIC_ORDER /* a dive pool: a slot of either walk */
                                                 : head.hi == CS_DIVE_CK_MAGIC || head.hi == CS_DIVE_CK_MAGIC_ALLOWED;
  if (!magic_ok || head.lo < 0 || head.lo >= ck->frames)
    return set_err(CSGPU_E_STATE, "slot %d holds no checkpoint", slot);
  if (head2 != NULL) { head2[0] = header[0]; head2[1] = header[1]; }
  *count = (int64_t)head.lo + 1;
  if (cap < *count)
    return set_err(CSGPU_E_LIMIT, "the checkpoint has %lld open subtrees, the buffer holds %lld", (long long)*count, (long long)cap);
  const int *root_lo_d = kind != MANY_POOL_DIVE ? ck->d_zero : ck->m->d_root_lo;
  hipLaunchKernelGGL(cs_dive_export, dim3((unsigned)*count), dim3(CS_WAVE), 0, (hipStream_t)stream, n, root_lo_d, base,
                     (cs_val *)d_states);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_many_checkpoint_states(const csgpu_many_checkpoints *ck, int32_t slot, csgpu_val *d_states, int64_t cap,
                                            int64_t *count, void *stream) {
  return many_pool_states(ck, MANY_POOL_DIVE, slot, d_states, cap, count, NULL, stream);
}

/* ---- stopped ALL walks spread over the next launch: their children counted, fanned out as root rows, folded back ---- */

#define MANY_FAN_LIMIT "more than 2^31 - 1 instances in one call"

extern "C" int csgpu_many_checkpoint_children(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                              int64_t *d_children, void *stream) {
  if (ck == NULL || d_slots == NULL || d_children == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (count < 0) return set_err(CSGPU_E_ARG, "negative instance count");
  if (ck->kind != MANY_POOL_DIVE) return set_err(CSGPU_E_ARG, MANY_POOL_KIND);
  if (count > 0x7fffffff) return set_err(CSGPU_E_LIMIT, MANY_FAN_LIMIT);
  if (count == 0) return CSGPU_OK;
  const csgpu_model *m = ck->m;
  const unsigned grid = (unsigned)((count + CS_DIVE_FAN_WAVES - 1) / CS_DIVE_FAN_WAVES);
  hipLaunchKernelGGL(cs_dive_children, dim3(grid), dim3(CS_DIVE_FAN_WAVES * CS_WAVE), 0, (hipStream_t)stream, m->host->n_vars,
                     (const int *)m->d_root_lo, (const int *)m->d_root_hi, (const cs_val *)ck->d_pool, (int)ck->capacity,
                     (const int *)d_slots, (long long)count, (long long *)d_children);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_many_checkpoint_fanout(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                            const int64_t *d_offsets, csgpu_val *d_rows, int32_t *d_owner, int64_t total,
                                            void *stream) {
  if (ck == NULL || d_slots == NULL || d_offsets == NULL || d_rows == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (count < 0) return set_err(CSGPU_E_ARG, "negative instance count");
  if (total < 0) return set_err(CSGPU_E_ARG, "negative row count");
  if (ck->kind != MANY_POOL_DIVE) return set_err(CSGPU_E_ARG, MANY_POOL_KIND);
  if (count > 0x7fffffff) return set_err(CSGPU_E_LIMIT, MANY_FAN_LIMIT);
  if (count == 0 || total == 0) return CSGPU_OK;
  const csgpu_model *m = ck->m;
  const unsigned grid = (unsigned)((count + CS_DIVE_FAN_WAVES - 1) / CS_DIVE_FAN_WAVES);
  hipLaunchKernelGGL(cs_dive_fanout, dim3(grid), dim3(CS_DIVE_FAN_WAVES * CS_WAVE), 0, (hipStream_t)stream, m->host->n_vars,
                     (const int *)m->d_root_lo, (const int *)m->d_root_hi, (const cs_val *)ck->d_pool, (int)ck->capacity,
                     (const int *)d_slots, (long long)count, (const long long *)d_offsets, (long long)total, (cs_val *)d_rows,
                     (int *)d_owner);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_many_fold(const csgpu_many_result *d_sub_results, const int32_t *d_owner, int64_t total,
                               csgpu_many_result *d_results, void *stream) {
  if (d_sub_results == NULL || d_owner == NULL || d_results == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (total < 0) return set_err(CSGPU_E_ARG, "negative record count");
  if (total > 256ll * 0x7fffffff) return set_err(CSGPU_E_LIMIT, "more than 2^39 - 256 records in one call");
  if (total == 0) return CSGPU_OK;
  hipLaunchKernelGGL(cs_dive_fold, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const cs_dive_result *)d_sub_results, (const int *)d_owner, (long long)total, (cs_dive_result *)d_results);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

/* ---- branching on the allowed values (cs_dive_allowed, cs_dive_allowed_upto): the plain walk and up to k ---- */

extern "C" int csgpu_model_qualifies_many_allowed(const csgpu_model *m) {
  if (m == NULL || !many_qualifies(m)) return 0;
  if (m->finalized) return m->plan.dive[MANY_ALLOWED].fn != NULL;
  return widest_root_domain(m) <= CS_DIVE_ALLOWED_WIDTH;
}

/* a model of csgpu_solve_many whose domains the allowed sets do not hold: said before many_check_tail's general refusal */
static int many_check_allowed_width(const csgpu_model *m) {
  if (m->finalized && m->plan.dive[MANY_PLAIN].fn != NULL && m->plan.dive[MANY_ALLOWED].fn == NULL)
    return set_err(CSGPU_E_LIMIT, "csgpu_solve_many_allowed: a root domain of this model has more than %d values, which is as wide "
                                  "as the allowed-value sets of the kernels are; csgpu_solve_many runs it",
                   CS_DIVE_ALLOWED_WIDTH);
  return CSGPU_OK;
}

extern "C" int csgpu_solve_many_allowed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                        const csgpu_many_options *options, csgpu_many_result *d_results, int32_t *d_solutions,
                                        void *stream) {
  const int null_arg = m == NULL || d_roots == NULL || d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "instance")) ||
      (rc = many_check_objective(options->objective)) || (rc = many_check_allowed_width(m)) ||
      (rc = many_check_tail(m, MANY_ALLOWED, NULL, count)))
    return rc;
  return many_launch(m, MANY_ALLOWED, d_roots, count, options->max_nodes, options->objective == CS_OBJ_ALL, d_results,
                     d_solutions, 0, stream, NULL, NULL);
}

extern "C" int csgpu_solve_many_allowed_upto(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                             const csgpu_many_upto_options *options, csgpu_many_result *d_results,
                                             int32_t *d_solutions, void *stream) {
  const int null_arg = m == NULL || d_roots == NULL || d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "instance"))) return rc;
  if (options->max_solutions < 1) return set_err(CSGPU_E_ARG, "max_solutions must be at least 1: an instance stops at its k-th solution");
  if ((rc = many_check_allowed_width(m)) || (rc = many_check_tail(m, MANY_ALLOWED_UPTO, NULL, count))) return rc;
  int upto = options->max_solutions;
  return many_launch(m, MANY_ALLOWED_UPTO, d_roots, count, options->max_nodes, 1 /* not read */, d_results, d_solutions, 0, stream,
                     &upto, NULL);
}

/* ---- the allowed walk with checkpoints (cs_dive_allowed_resume, cs_dive_allowed_upto_resume), and its spread ---- */

/* csgpu_solve_many_allowed_checkpointed, and with `resume` (and no roots) csgpu_solve_many_allowed_resume: the checks of
 * many_ck_call in its order, the width of the domains before the general refusal */
static int many_allowed_ck_call(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_options *options,
                                csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                int resume, void *stream) {
  const int null_arg = m == NULL || (!resume && d_roots == NULL) || d_results == NULL || options == NULL || ck == NULL || d_slots == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "slice")) ||
      (rc = many_check_objective(options->objective)) || (rc = many_check_allowed_width(m)) ||
      (rc = many_check_tail(m, MANY_ALLOWED_CK, ck, count)))
    return rc;
  cs_dive_ck dk = many_ck_arg(ck, d_slots, resume);
  return many_launch(m, MANY_ALLOWED_CK, d_roots, count, options->max_nodes, options->objective == CS_OBJ_ALL, d_results,
                     d_solutions, resume, stream, &dk, NULL);
}

extern "C" int csgpu_solve_many_allowed_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                                     const csgpu_many_options *options, csgpu_many_result *d_results,
                                                     int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                                     void *stream) {
  return many_allowed_ck_call(m, d_roots, count, options, d_results, d_solutions, ck, d_slots, 0, stream);
}

extern "C" int csgpu_solve_many_allowed_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options,
                                               csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck,
                                               int32_t *d_slots, void *stream) {
  return many_allowed_ck_call(m, NULL, count, options, d_results, d_solutions, ck, d_slots, 1, stream);
}

/* the two up-to-k calls: the checks of many_upto_call (pooled) in its order */
static int many_allowed_upto_ck_call(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                     const csgpu_many_upto_options *options, csgpu_many_result *d_results, int32_t *d_solutions,
                                     csgpu_many_checkpoints *ck, int32_t *d_slots, int resume, void *stream) {
  const int null_arg = m == NULL || (!resume && d_roots == NULL) || d_results == NULL || options == NULL || ck == NULL || d_slots == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "instance"))) return rc;
  if (options->max_solutions < 1) return set_err(CSGPU_E_ARG, "max_solutions must be at least 1: an instance stops at its k-th solution");
  if ((rc = many_check_allowed_width(m)) || (rc = many_check_tail(m, MANY_ALLOWED_UPTO_CK, ck, count))) return rc;
  cs_dive_ck dk = many_ck_arg(ck, d_slots, resume);
  int upto = options->max_solutions;
  return many_launch(m, MANY_ALLOWED_UPTO_CK, d_roots, count, options->max_nodes, 1 /* not read */, d_results, d_solutions, resume,
                     stream, &dk, &upto);
}

extern "C" int csgpu_solve_many_allowed_upto_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                                          const csgpu_many_upto_options *options, csgpu_many_result *d_results,
                                                          int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                                          void *stream) {
  return many_allowed_upto_ck_call(m, d_roots, count, options, d_results, d_solutions, ck, d_slots, 0, stream);
}

extern "C" int csgpu_solve_many_allowed_upto_resume(const csgpu_model *m, int64_t count, const csgpu_many_upto_options *options,
                                                    csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck,
                                                    int32_t *d_slots, void *stream) {
  return many_allowed_upto_ck_call(m, NULL, count, options, d_results, d_solutions, ck, d_slots, 1, stream);
}

/* the pool's model runs csgpu_solve_many (the pool exists) but not the allowed walk: its domains are too wide */
static int many_fan_allowed_width(const csgpu_many_checkpoints *ck) {
  if (ck->m->plan.dive[MANY_ALLOWED_CK].fn == NULL)
    return set_err(CSGPU_E_LIMIT, "csgpu_solve_many_allowed: a root domain of this model has more than %d values, which is as wide "
                                  "as the allowed-value sets of the kernels are; csgpu_solve_many runs it",
                   CS_DIVE_ALLOWED_WIDTH);
  return CSGPU_OK;
}

extern "C" int csgpu_many_allowed_checkpoint_children(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                      int64_t *d_children, void *stream) {
  if (ck == NULL || d_slots == NULL || d_children == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (count < 0) return set_err(CSGPU_E_ARG, "negative instance count");
  if (ck->kind != MANY_POOL_DIVE) return set_err(CSGPU_E_ARG, MANY_POOL_KIND);
  if (count > 0x7fffffff) return set_err(CSGPU_E_LIMIT, MANY_FAN_LIMIT);
  if (count == 0) return CSGPU_OK;
  int rc;
  if ((rc = many_fan_allowed_width(ck))) return rc; /* (after the empty call, which looks into no pool) */
  const csgpu_model *m = ck->m;
  const unsigned grid = (unsigned)((count + CS_DIVE_FAN_WAVES - 1) / CS_DIVE_FAN_WAVES);
  const int n = m->host->n_vars, slots = m->img->dense_slots, dmin = m->img->dense_dmin, cols = m->img->dense_cols;
#define CS_FAN(E)                                                                                                             \
  hipLaunchKernelGGL(cs_dive_allowed_children<E>, dim3(grid), dim3(CS_DIVE_FAN_WAVES * CS_WAVE), 0, (hipStream_t)stream, n,    \
                     (const int *)m->d_root_lo, (const int *)m->d_root_hi, (const E *)m->d_dense_tab, slots, dmin, cols,       \
                     (const cs_val *)ck->d_pool, (int)ck->capacity, (const int *)d_slots, (long long)count, (long long *)d_children)
  if (m->img->dense_width == 1) CS_FAN(unsigned char); else CS_FAN(unsigned short);
#undef CS_FAN
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_many_allowed_checkpoint_fanout(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                    const int64_t *d_offsets, csgpu_val *d_rows, int32_t *d_owner, int64_t total,
                                                    void *stream) {
  if (ck == NULL || d_slots == NULL || d_offsets == NULL || d_rows == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (count < 0) return set_err(CSGPU_E_ARG, "negative instance count");
  if (total < 0) return set_err(CSGPU_E_ARG, "negative row count");
  if (ck->kind != MANY_POOL_DIVE) return set_err(CSGPU_E_ARG, MANY_POOL_KIND);
  if (count > 0x7fffffff) return set_err(CSGPU_E_LIMIT, MANY_FAN_LIMIT);
  if (count == 0 || total == 0) return CSGPU_OK;
  int rc;
  if ((rc = many_fan_allowed_width(ck))) return rc;
  const csgpu_model *m = ck->m;
  const unsigned grid = (unsigned)((count + CS_DIVE_FAN_WAVES - 1) / CS_DIVE_FAN_WAVES);
  const int n = m->host->n_vars, slots = m->img->dense_slots, dmin = m->img->dense_dmin, cols = m->img->dense_cols;
#define CS_FAN(E)                                                                                                             \
  hipLaunchKernelGGL(cs_dive_allowed_fanout<E>, dim3(grid), dim3(CS_DIVE_FAN_WAVES * CS_WAVE), 0, (hipStream_t)stream, n,      \
                     (const int *)m->d_root_lo, (const int *)m->d_root_hi, (const E *)m->d_dense_tab, slots, dmin, cols,       \
                     (const cs_val *)ck->d_pool, (int)ck->capacity, (const int *)d_slots, (long long)count,                    \
                     (const long long *)d_offsets, (long long)total, (cs_val *)d_rows, (int *)d_owner)
  if (m->img->dense_width == 1) CS_FAN(unsigned char); else CS_FAN(unsigned short);
#undef CS_FAN
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

/* ---- up to k solutions per instance (cs_dive_upto): csgpu_solve_many, stopped at the k-th solution, all k rows kept ---- */

/* the three calls.  `pooled`: the call has a pool and slot numbers; `resume` (pooled, and no roots): it goes on in them */
static int many_upto_call(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_upto_options *options,
                          csgpu_many_result *d_results, int32_t *d_solutions, int pooled, csgpu_many_checkpoints *ck,
                          int32_t *d_slots, int resume, void *stream) {
  const int null_arg = m == NULL || (!resume && d_roots == NULL) || d_results == NULL || options == NULL ||
                       (pooled && (ck == NULL || d_slots == NULL));
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "instance"))) return rc;
  if (options->max_solutions < 1) return set_err(CSGPU_E_ARG, "max_solutions must be at least 1: an instance stops at its k-th solution");
  if ((rc = many_check_tail(m, MANY_UPTO, ck, count))) return rc;
  cs_dive_ck dk = many_ck_arg(ck, d_slots, resume);
  int upto = options->max_solutions;
  return many_launch(m, MANY_UPTO, d_roots, count, options->max_nodes, 1 /* not read: the ALL walk, left at the k-th solution */,
                     d_results, d_solutions, resume, stream, &dk, &upto);
}

extern "C" int csgpu_solve_many_upto(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                     const csgpu_many_upto_options *options, csgpu_many_result *d_results, int32_t *d_solutions,
                                     void *stream) {
  return many_upto_call(m, d_roots, count, options, d_results, d_solutions, 0, NULL, NULL, 0, stream);
}

extern "C" int csgpu_solve_many_upto_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                                  const csgpu_many_upto_options *options, csgpu_many_result *d_results,
                                                  int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                                  void *stream) {
  return many_upto_call(m, d_roots, count, options, d_results, d_solutions, 1, ck, d_slots, 0, stream);
}

extern "C" int csgpu_solve_many_upto_resume(const csgpu_model *m, int64_t count, const csgpu_many_upto_options *options,
                                            csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck,
                                            int32_t *d_slots, void *stream) {
  return many_upto_call(m, NULL, count, options, d_results, d_solutions, 1, ck, d_slots, 1, stream);
}

/* ---- Luby restarts with a seeded value order for ANY (cs_dive_restart) ---- */

extern "C" int csgpu_solve_many_restarts(const csgpu_model *m, const csgpu_val *d_roots, const uint32_t *d_seeds, int64_t count,
                                         const csgpu_many_restart_options *options, csgpu_many_result *d_results,
                                         int32_t *d_solutions, int32_t *d_restarts, void *stream) {
  const int null_arg = m == NULL || d_roots == NULL || d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "instance"))) return rc;
  if (options->restart_base < 0) return set_err(CSGPU_E_ARG, "restart_base must not be negative (0: no restarts)");
  if ((options->flags & ~CSGPU_MANY_ROTATE_FIRST) != 0) return set_err(CSGPU_E_ARG, "unknown flags 0x%x", (unsigned)options->flags);
  if ((rc = many_check_tail(m, MANY_RESTART, NULL, count))) return rc;
  cs_dive_rs rs;
  rs.seeds = d_seeds;
  rs.restarts = d_restarts;
  rs.restart_base = (long long)options->restart_base;
  rs.seed = options->seed;
  rs.flags = options->flags;
  return many_launch(m, MANY_RESTART, d_roots, count, options->max_nodes, 0, d_results, d_solutions, 0, stream, &rs, NULL);
}

/* ---- every solution of every instance under ALL, through one bounded stream (cs_dive_stream) ---- */

extern "C" int csgpu_solve_many_stream(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                       const csgpu_many_options *options, csgpu_many_result *d_results,
                                       csgpu_many_checkpoints *ck, int32_t *d_slots, const csgpu_many_stream *out, void *stream) {
  const int null_arg = m == NULL || d_roots == NULL || d_results == NULL || options == NULL || ck == NULL || d_slots == NULL ||
                       out == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "call"))) return rc;
  if (options->objective != CS_OBJ_ALL)
    return set_err(CSGPU_E_ARG, "csgpu_solve_many_stream walks under ALL (objective 1), not objective %d", options->objective);
  if (out->capacity < 1) return set_err(CSGPU_E_ARG, "the solution stream has room for at least one row (capacity %lld)", (long long)out->capacity);
  if (out->d_rows == NULL || out->d_owner == NULL || out->d_count == NULL) return set_err(CSGPU_E_ARG, "null pointer in the solution stream");
  if ((rc = many_check_tail(m, MANY_STREAM, ck, count))) return rc;
  cs_dive_ck dk = many_ck_arg(ck, d_slots, 0); /* fresh or resumed is d_slots[i]'s to say: the kernel does not read `resume` */
  cs_dive_out ok;
  ok.rows = out->d_rows;
  ok.owner = out->d_owner;
  ok.count = (unsigned long long *)out->d_count;
  ok.capacity = (long long)out->capacity;
  return many_launch(m, MANY_STREAM, d_roots, count, options->max_nodes, 1, d_results, NULL, 0, stream, &dk, &ok);
}

/* ---- clause models: csgpu_solve_many_clauses, a depth-first search per wavefront on kernel 6's fixpoint (cs_walk.hip.h) ---- */

#define MANY_CLAUSES_STACK_MAX ((size_t)1 << 30) /* bytes of frames a call keeps: fewer waves rather than more memory */

extern "C" int csgpu_model_qualifies_many_clauses(const csgpu_model *m) {
  return m != NULL && m->finalized && m->plan.walk[WALK_PLAIN].fn != NULL;
}

/* waves a call with `count` instances launches: the resident ones, no more than the instances need, and no more than
 * whose `frames` frames each fit MANY_CLAUSES_STACK_MAX (one workgroup's always do: n is at most 5118 where four slices
 * fit a CU) */
static int64_t many_clauses_waves(const csgpu_model *m, const cs_planned *k, int64_t count, int frames) {
  const size_t n = (size_t)m->host->n_vars;
  int64_t grid = (int64_t)m->n_cus * k->per_cu;
  const int64_t by_count = (count + k->waves - 1) / k->waves;
  const int64_t by_stack = (int64_t)(MANY_CLAUSES_STACK_MAX / ((size_t)k->waves * (size_t)frames * (n + 1) * sizeof(cs_val)));
  if (grid > by_count) grid = by_count;
  if (grid > by_stack) grid = by_stack;
  if (grid < 1) grid = 1;
  return grid * k->waves;
}

extern "C" int64_t csgpu_internal_many_clauses_waves(const csgpu_model *m, int64_t count) {
  if (!csgpu_model_qualifies_many_clauses(m) || count < 1) return 0;
  return many_clauses_waves(m, &m->plan.walk[WALK_PLAIN], count, m->host->n_vars);
}

/* The frames a wave of cs_walk_order needs, from the root domains alone: n + sum of h(v), h(v) the smallest h for which
 * the root width of v, halved h times with ceiling, is at most split_width.  A pushed frame is a parent with children
 * left: one that enumerates has valued a variable in the child it waits for (at most n - 1 of those along a path, and the
 * current node's frame), one that halves waits for its second half while its first, of at most ceil(width / 2) values,
 * is walked -- at most h(v) of those per variable, since rows lie inside the root domains and intervals only shrink. */
static int64_t many_clauses_ordered_frames(const csgpu_model *m, int32_t split_width) {
  const int64_t split = split_width == 0 ? 256 : (int64_t)split_width;
  int64_t frames = m->host->n_vars;
  for (int32_t v = 0; v < m->host->n_vars; v++) {
    int64_t w = (int64_t)m->host->dom[v].hi - (int64_t)m->host->dom[v].lo + 1;
    for (; w > split; w = (w + 1) >> 1) frames++;
  }
  return frames;
}

extern "C" int64_t csgpu_many_clauses_ordered_frames(const csgpu_model *m, int32_t split_width) {
  if (!csgpu_model_qualifies_many_clauses(m) || split_width < 0) return 0;
  return many_clauses_ordered_frames(m, split_width);
}

/* The checks of every clause entry, none of which touches the device: many_check_head, the entry's own checks of its
 * options (and the stream's of its stream), many_clauses_check_model, what the start and the ordered entries add, and
 * many_clauses_check_pool for a call that has a pool.  This one: the objective the call walks under, against the model;
 * then the model and the count.  The objective's half stands alone for the wide entries, whose model check is their own. */
static int many_clauses_check_objective(const csgpu_model *m, int objective) {
  if (objective != CS_OBJ_ANY && objective != CS_OBJ_ALL && objective != CS_OBJ_MIN && objective != CS_OBJ_MAX)
    return set_err(CSGPU_E_ARG, "no objective %d", objective);
  if (objective == CS_OBJ_MIN || objective == CS_OBJ_MAX) {
    if (m->host->obj_var < 0 || m->host->obj_var >= m->host->n_vars)
      return set_err(CSGPU_E_ARG, "MIN / MAX need a model with an objective: this one has none");
    if (m->host->objective != objective)
      return set_err(CSGPU_E_ARG, "the model's objective is %s: it cannot be searched with %s",
                     m->host->objective == CS_OBJ_MIN ? "MIN" : "MAX", objective == CS_OBJ_MIN ? "MIN" : "MAX");
  }
  return CSGPU_OK;
}

static int many_clauses_check_model(const csgpu_model *m, int objective, int64_t count) {
  int rc;
  if ((rc = many_clauses_check_objective(m, objective))) return rc;
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (m->plan.walk[WALK_PLAIN].fn == NULL) {
    if (m->plan.rounds_cpl == 0)
      return set_err(CSGPU_E_LIMIT, "model does not qualify for the clause-resident kernel (at most 512 clauses; this one has %d), "
                                    "which csgpu_solve_many_clauses is built on", (int)m->img->n_clauses);
    return set_err(CSGPU_E_LIMIT, "csgpu_solve_many_clauses: %d variables make LDS slices of %zu bytes for the %d waves of a "
                                  "workgroup, more than the 160 KiB of a CU", (int)m->host->n_vars, m->plan.rounds.lds, CS_WAVES_PER_BLOCK);
  }
  if (count > 0x7fffffff - CS_DIVE_SHARDS) return set_err(CSGPU_E_LIMIT, "more than 2^31 - 65 instances in one call");
  return CSGPU_OK;
}

/* what the caller of an entry brought (the trailing ones NULL where the entry has none) */
struct many_clauses_bufs {
  const csgpu_val *d_roots; /* NULL: a resume */
  int64_t count;
  csgpu_many_result *d_results;
  void *stream;
  int32_t *d_solutions;
  int32_t *d_best; /* read under MIN / MAX alone */
  csgpu_many_checkpoints *ck;
  int32_t *d_slots;
};

/* `kind`: MANY_POOL_WALK, the ordered entries' MANY_POOL_ORDER, which take no pool of either older kind, or the wide
 * entries' MANY_POOL_WIDE, which take no other either */
static int many_clauses_check_pool(const csgpu_model *m, const many_clauses_bufs *b, int kind) {
  if (b->ck == NULL || b->d_slots == NULL) return set_err(CSGPU_E_ARG, "null argument: a checkpointed call has a pool and slot numbers");
  if (b->ck->m != m) return set_err(CSGPU_E_ARG, "the checkpoint pool was created for another model");
  if (b->ck->kind != kind)
    return set_err(CSGPU_E_ARG, kind == MANY_POOL_ORDER ? MANY_POOL_KIND_ORDER : kind == MANY_POOL_WIDE ? MANY_POOL_KIND_WIDE : MANY_POOL_KIND);
  return CSGPU_OK;
}

/* the pool and slot numbers as the kernels take them, `code` in the header of every checkpoint the call writes or goes on
 * from; without a pool: one of capacity 0 that cs_walk_upto and cs_walk_from do not touch */
static cs_walk_ck many_clauses_ck_arg(const many_clauses_bufs *b, int resume, int code) {
  cs_walk_ck wk;
  wk.pool = b->ck != NULL ? b->ck->d_pool : NULL;
  wk.next = b->ck != NULL ? b->ck->d_next : NULL;
  wk.capacity = b->ck != NULL ? (int)b->ck->capacity : 0;
  wk.resume = resume;
  wk.code = code;
  wk.slots = b->ck != NULL ? b->d_slots : NULL;
  return wk;
}


/* The one launch of a cs_walk_* kernel, after the checks.  `frames` per wave: at most n - 1 pushed frames and the current
 * node's; cs_walk_restart: and the root node's; cs_walk_order: and the halving parents' (at most 33 n, n <= 5118: an int).
 * `tail0` .. `tail2`: the family's own kernel arguments after the tables and the cs_walk_io (NULL where it has fewer).
 * `resume`: the instances go on in the frames of their checkpoint slots, so the call brings no roots and needs no stacks. */
static int many_clauses_launch(const csgpu_model *m, int family, int frames, int objective, int64_t max_nodes,
                               const many_clauses_bufs *b, int resume, void *tail0, void *tail1, void *tail2) {
  if (b->count == 0) return CSGPU_OK;
  csgpu_model *mm = const_cast<csgpu_model *>(m);
  const cs_planned *k = &m->plan.walk[family];
  const int64_t waves = many_clauses_waves(m, k, b->count, frames);
  int rc;
  if ((rc = many_workspace(mm, resume ? 0 : waves, frames))) return rc;
  cs_walk_io io;
  io.roots = (const cs_val *)b->d_roots;
  io.root_dom = m->d_walk_root;
  io.count = (int)b->count;
  io.all = objective != CS_OBJ_ANY;
  io.sense = objective_sense(objective);
  io.obj_var = io.sense != 0 ? m->host->obj_var : -1;
  io.max_nodes = (long long)max_nodes;
  io.results = (cs_dive_result *)b->d_results;
  io.solutions = b->d_solutions;
  io.best = io.sense != 0 ? b->d_best : NULL;
  io.stack = resume ? NULL : (cs_val *)mm->d_many_stack;
  io.frames = frames;
  io.tickets = mm->d_many_tickets;
  cs_tables tab = m->tab;
  void *args[] = { &tab, &io, tail0, tail1, tail2 };
  HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)(waves / k->waves)), dim3((unsigned)(k->waves * CS_WAVE)), args, k->lds,
                          (hipStream_t)b->stream));
  return CSGPU_OK;
}

extern "C" int csgpu_solve_many_clauses(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                        const csgpu_many_options *options, csgpu_many_result *d_results, int32_t *d_solutions,
                                        int32_t *d_best, void *stream) {
  const int null_arg = m == NULL || d_roots == NULL || d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "instance")) ||
      (rc = many_clauses_check_model(m, options->objective, count)))
    return rc;
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions, d_best };
  return many_clauses_launch(m, WALK_PLAIN, m->host->n_vars, options->objective, options->max_nodes, &b, 0, NULL, NULL, NULL);
}


/* ---- clause checkpoints: csgpu_solve_many_clauses in slices (cs_walk_resume) ---- */

/* does the model run the cs_walk_* kernels?  What finalize planned; before finalize, the same rules on the host tables
 * (csgpu_model_build_tables) as they stand */
static int many_clauses_qualifies(const csgpu_model *m) {
  if (m->finalized) return m->plan.walk[WALK_PLAIN].fn != NULL;
  if (m->img == NULL) return 0;
  const size_t slice = ((size_t)m->host->n_vars * sizeof(cs_val) + 16 + 15) & ~(size_t)15;
  return m->img->n_clauses > 0 && m->img->n_clauses <= 8 * CS_WAVE && slice * CS_WAVES_PER_BLOCK <= CS_CU_LDS;
}

extern "C" size_t csgpu_many_clause_checkpoint_bytes(const csgpu_model *m) {
  if (m == NULL || !many_clauses_qualifies(m)) return 0;
  const size_t n = (size_t)m->host->n_vars;
  return (n + 1) * (n + 1) * sizeof(cs_val); /* the header frame, n - 1 pushed frames at most, the current node */
}

extern "C" int csgpu_many_clause_checkpoints_create(const csgpu_model *m, int64_t capacity, csgpu_many_checkpoints **out) {
  return many_pool_create(m, capacity, MANY_POOL_WALK, csgpu_model_qualifies_many_clauses(m),
                          "model does not qualify for csgpu_solve_many_clauses (kernel 6 planned, its LDS slices fit a CU)",
                          csgpu_many_clause_checkpoint_bytes(m), m != NULL ? m->host->n_vars : 0, 0, out);
}

/* the checkpointed call and its resume (no roots): cs_walk_resume under the options' objective, which is the checkpoints' code */
static int many_clauses_pooled(const csgpu_model *m, const many_clauses_bufs *b, const csgpu_many_options *options, int resume) {
  const int null_arg = m == NULL || (!resume && b->d_roots == NULL) || b->d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, b->count, null_arg ? 0 : options->max_nodes, "slice")) ||
      (rc = many_clauses_check_model(m, options->objective, b->count)) || (rc = many_clauses_check_pool(m, b, MANY_POOL_WALK)))
    return rc;
  cs_walk_ck wk = many_clauses_ck_arg(b, resume, options->objective);
  return many_clauses_launch(m, WALK_CK, m->host->n_vars, options->objective, options->max_nodes, b, resume, &wk, NULL, NULL);
}

extern "C" int csgpu_solve_many_clauses_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                                     const csgpu_many_options *options, csgpu_many_result *d_results,
                                                     int32_t *d_solutions, int32_t *d_best, csgpu_many_checkpoints *ck,
                                                     int32_t *d_slots, void *stream) {
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_clauses_pooled(m, &b, options, 0);
}

extern "C" int csgpu_solve_many_clauses_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options,
                                               csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                               csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream) {
  const many_clauses_bufs b = { NULL, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_clauses_pooled(m, &b, options, 1);
}

extern "C" int csgpu_many_clause_checkpoint_states(const csgpu_many_checkpoints *ck, int32_t slot, csgpu_val *d_states, int64_t cap,
                                                   int64_t *count, int32_t *best, int32_t *have_best, void *stream) {
  if (best == NULL || have_best == NULL) return set_err(CSGPU_E_ARG, "null argument");
  cs_val header[2] = { cs_interval(0, 0), cs_interval(0, 0) };
  /* a pool of either clause kind: an ordered one has the same frames, more of them, under its own magic */
  const int kind = ck != NULL && ck->kind == MANY_POOL_ORDER ? MANY_POOL_ORDER : MANY_POOL_WALK;
  const int rc = many_pool_states(ck, kind, slot, d_states, cap, count, header, stream);
  if (rc == CSGPU_OK || rc == CSGPU_E_LIMIT) { /* (a buffer too small: *count and the incumbent are set all the same) */
    *best = header[1].lo;
    *have_best = header[1].hi & 1;
  }
  return rc;
}

/* ---- clause models past 512 clauses: csgpu_solve_many_clauses_wide, the records in LDS (cs_walk_wide, cs_walk_wide_resume) ---- */

/* does the model run the cs_walk_wide kernels?  What finalize planned; before finalize, the same rule on the host tables
 * (csgpu_model_build_tables) as they stand.  `bytes`, if wanted: the LDS a workgroup needs (0 without tables) */
static int many_wide_qualifies(const csgpu_model *m, size_t *bytes) {
  if (bytes != NULL) *bytes = 0;
  if (m->img == NULL) return 0;
  const size_t lds = m->finalized ? many_wide_lds(m->host->n_vars, m->tab.n_clauses, m->tab.n_lits)
                                  : many_wide_lds(m->host->n_vars, m->img->n_clauses, m->img->n_lits);
  if (bytes != NULL) *bytes = lds;
  if (m->finalized) return m->plan.walk[WALK_WIDE].fn != NULL;
  return m->img->n_clauses > 0 && lds <= CS_CU_LDS;
}

extern "C" int csgpu_model_qualifies_many_clauses_wide(const csgpu_model *m) {
  return m != NULL && many_wide_qualifies(m, NULL);
}

extern "C" size_t csgpu_many_clause_wide_checkpoint_bytes(const csgpu_model *m) {
  if (m == NULL || !many_wide_qualifies(m, NULL)) return 0;
  const size_t n = (size_t)m->host->n_vars;
  return (n + 1) * (n + 1) * sizeof(cs_val); /* cs_walk_resume's slot: the header frame, n - 1 pushed frames at most, the current node */
}

extern "C" int csgpu_many_clause_wide_checkpoints_create(const csgpu_model *m, int64_t capacity, csgpu_many_checkpoints **out) {
  return many_pool_create(m, capacity, MANY_POOL_WIDE, m != NULL && m->finalized && m->plan.walk[WALK_WIDE_CK].fn != NULL,
                          "model does not qualify for csgpu_solve_many_clauses_wide (a clause, and its records and LDS slices fit a CU)",
                          csgpu_many_clause_wide_checkpoint_bytes(m), m != NULL ? m->host->n_vars : 0, 0, out);
}

/* the one model check of the wide entries: many_clauses_check_model's objective checks, then the model and the count */
static int many_wide_check_model(const csgpu_model *m, int objective, int64_t count) {
  int rc;
  if ((rc = many_clauses_check_objective(m, objective))) return rc;
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (m->plan.walk[WALK_WIDE].fn == NULL) {
    size_t bytes = 0;
    (void)many_wide_qualifies(m, &bytes);
    if (m->tab.n_clauses <= 0) return set_err(CSGPU_E_LIMIT, "csgpu_solve_many_clauses_wide walks on clause records: this model has none");
    return set_err(CSGPU_E_LIMIT, "csgpu_solve_many_clauses_wide: %d clause and %d literal records and the LDS slices of the %d waves "
                                  "of a workgroup need %zu bytes of LDS, more than the 160 KiB (%u bytes) of a CU",
                   (int)m->tab.n_clauses, (int)m->tab.n_lits, CS_WAVES_PER_BLOCK, bytes, CS_CU_LDS);
  }
  if (count > 0x7fffffff - CS_DIVE_SHARDS) return set_err(CSGPU_E_LIMIT, "more than 2^31 - 65 instances in one call");
  return CSGPU_OK;
}

extern "C" int csgpu_solve_many_clauses_wide(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                             const csgpu_many_options *options, csgpu_many_result *d_results,
                                             int32_t *d_solutions, int32_t *d_best, void *stream) {
  const int null_arg = m == NULL || d_roots == NULL || d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "instance")) ||
      (rc = many_wide_check_model(m, options->objective, count)))
    return rc;
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions, d_best };
  return many_clauses_launch(m, WALK_WIDE, m->host->n_vars, options->objective, options->max_nodes, &b, 0, NULL, NULL, NULL);
}

/* the checkpointed call and its resume (no roots): cs_walk_wide_resume under the options' objective, the checkpoints' code */
static int many_wide_pooled(const csgpu_model *m, const many_clauses_bufs *b, const csgpu_many_options *options, int resume) {
  const int null_arg = m == NULL || (!resume && b->d_roots == NULL) || b->d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, b->count, null_arg ? 0 : options->max_nodes, "slice")) ||
      (rc = many_wide_check_model(m, options->objective, b->count)) || (rc = many_clauses_check_pool(m, b, MANY_POOL_WIDE)))
    return rc;
  cs_walk_ck wk = many_clauses_ck_arg(b, resume, options->objective);
  return many_clauses_launch(m, WALK_WIDE_CK, m->host->n_vars, options->objective, options->max_nodes, b, resume, &wk, NULL, NULL);
}

extern "C" int csgpu_solve_many_clauses_wide_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                                          const csgpu_many_options *options, csgpu_many_result *d_results,
                                                          int32_t *d_solutions, int32_t *d_best, csgpu_many_checkpoints *ck,
                                                          int32_t *d_slots, void *stream) {
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_wide_pooled(m, &b, options, 0);
}

extern "C" int csgpu_solve_many_clauses_wide_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options,
                                                    csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                                    csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream) {
  const many_clauses_bufs b = { NULL, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_wide_pooled(m, &b, options, 1);
}

extern "C" int64_t csgpu_internal_many_clauses_wide_waves(const csgpu_model *m, int64_t count) {
  if (m == NULL || !m->finalized || m->plan.walk[WALK_WIDE].fn == NULL || count < 1) return 0;
  return many_clauses_waves(m, &m->plan.walk[WALK_WIDE], count, m->host->n_vars);
}

/* ---- stopped ALL walks of a clause model spread over the next launch (cs_walk_children, cs_walk_fanout); the fold is
 * csgpu_many_fold, which works on records alone ---- */

/* the two calls and their _obj forms: `code`, the header code the checkpoints must carry; d_start (the _obj fan-out):
 * where every row's start incumbent goes, d_owner_start: NULL or what the owners hold */
static int many_clause_children(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count, int code,
                                int64_t *d_children, void *stream) {
  if (ck == NULL || d_slots == NULL || d_children == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (count < 0) return set_err(CSGPU_E_ARG, "negative instance count");
  if (ck->kind != MANY_POOL_WALK) return set_err(CSGPU_E_ARG, MANY_POOL_KIND);
  if (count > 0x7fffffff) return set_err(CSGPU_E_LIMIT, MANY_FAN_LIMIT);
  if (count == 0) return CSGPU_OK;
  const csgpu_model *m = ck->m;
  const unsigned grid = (unsigned)((count + CS_DIVE_FAN_WAVES - 1) / CS_DIVE_FAN_WAVES);
  hipLaunchKernelGGL(cs_walk_children, dim3(grid), dim3(CS_DIVE_FAN_WAVES * CS_WAVE), 0, (hipStream_t)stream, m->host->n_vars,
                     (const cs_val *)m->d_walk_root, (const cs_val *)ck->d_pool, (int)ck->capacity, (const int *)d_slots,
                     (long long)count, (long long *)d_children, code);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

static int many_clause_fanout(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count, int code,
                              const csgpu_many_start *d_owner_start, const int64_t *d_offsets, csgpu_val *d_rows,
                              int32_t *d_owner, csgpu_many_start *d_start, int64_t total, void *stream) {
  if (ck == NULL || d_slots == NULL || d_offsets == NULL || d_rows == NULL || (code != CS_WALK_CK_ALL && d_start == NULL))
    return set_err(CSGPU_E_ARG, "null argument");
  if (count < 0) return set_err(CSGPU_E_ARG, "negative instance count");
  if (total < 0) return set_err(CSGPU_E_ARG, "negative row count");
  if (ck->kind != MANY_POOL_WALK) return set_err(CSGPU_E_ARG, MANY_POOL_KIND);
  if (count > 0x7fffffff) return set_err(CSGPU_E_LIMIT, MANY_FAN_LIMIT);
  if (count == 0 || total == 0) return CSGPU_OK;
  const csgpu_model *m = ck->m;
  const unsigned grid = (unsigned)((count + CS_DIVE_FAN_WAVES - 1) / CS_DIVE_FAN_WAVES);
  hipLaunchKernelGGL(cs_walk_fanout, dim3(grid), dim3(CS_DIVE_FAN_WAVES * CS_WAVE), 0, (hipStream_t)stream, m->host->n_vars,
                     (const cs_val *)m->d_walk_root, (const cs_val *)ck->d_pool, (int)ck->capacity, (const int *)d_slots,
                     (long long)count, (const long long *)d_offsets, (long long)total, (cs_val *)d_rows, (int *)d_owner, code,
                     (const cs_walk_start *)d_owner_start, (cs_walk_start *)d_start);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_many_clause_checkpoint_children(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                     int64_t *d_children, void *stream) {
  return many_clause_children(ck, d_slots, count, CS_WALK_CK_ALL, d_children, stream);
}

extern "C" int csgpu_many_clause_checkpoint_fanout(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                   const int64_t *d_offsets, csgpu_val *d_rows, int32_t *d_owner, int64_t total,
                                                   void *stream) {
  return many_clause_fanout(ck, d_slots, count, CS_WALK_CK_ALL, NULL, d_offsets, d_rows, d_owner, NULL, total, stream);
}

/* ---- an instance that starts with an incumbent it did not find itself, and stopped MIN / MAX walks spread with it
 * (cs_walk_from; cs_walk_children / cs_walk_fanout with MIN's or MAX's code; cs_walk_fold_best) ---- */

/* the start call, checkpointed with a pool and slot numbers and plain with neither, and its resume (no roots, no starts:
 * the slots hold the incumbents), which is checkpointed: cs_walk_from under MIN / MAX.  What the two refuse comes after
 * csgpu_solve_many_clauses's own errors: the start, the objective, then the pool and the slots together */
static int many_clauses_from(const csgpu_model *m, const many_clauses_bufs *b, const csgpu_many_start *d_start,
                             const csgpu_many_options *options, int resume) {
  const int null_arg = m == NULL || (!resume && b->d_roots == NULL) || b->d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, b->count, null_arg ? 0 : options->max_nodes, resume ? "slice" : "instance")) ||
      (rc = many_clauses_check_model(m, options->objective, b->count)))
    return rc;
  if (!resume && d_start == NULL) return set_err(CSGPU_E_ARG, "null argument: d_start, the incumbents the instances start with");
  if (options->objective != CS_OBJ_MIN && options->objective != CS_OBJ_MAX)
    return set_err(CSGPU_E_ARG, "a start incumbent bounds a MIN / MAX walk (objective 2 or 3), not objective %d", options->objective);
  if ((b->ck == NULL) != (b->d_slots == NULL))
    return set_err(CSGPU_E_ARG, "null argument: a checkpointed call has a pool and slot numbers, a plain one neither");
  if (resume && b->ck == NULL) return set_err(CSGPU_E_ARG, "null argument: a checkpointed call has a pool and slot numbers");
  if (b->ck != NULL && (rc = many_clauses_check_pool(m, b, MANY_POOL_WALK))) return rc;
  cs_walk_ck wk = many_clauses_ck_arg(b, resume, options->objective);
  const cs_walk_start *starts = (const cs_walk_start *)d_start;
  return many_clauses_launch(m, WALK_FROM, m->host->n_vars, options->objective, options->max_nodes, b, resume, &wk, &starts, NULL);
}

extern "C" int csgpu_solve_many_clauses_from(const csgpu_model *m, const csgpu_val *d_roots, const csgpu_many_start *d_start,
                                             int64_t count, const csgpu_many_options *options, csgpu_many_result *d_results,
                                             int32_t *d_solutions, int32_t *d_best, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                             void *stream) {
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_clauses_from(m, &b, d_start, options, 0);
}

extern "C" int csgpu_solve_many_clauses_from_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options,
                                                    csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                                    csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream) {
  const many_clauses_bufs b = { NULL, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_clauses_from(m, &b, NULL, options, 1);
}

#define MANY_OBJ_CODE "the checkpoints of a MIN or a MAX walk are asked for (objective 2 or 3), not objective %d"

extern "C" int csgpu_many_clause_checkpoint_children_obj(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                         int objective, int64_t *d_children, void *stream) {
  if (objective != CS_OBJ_MIN && objective != CS_OBJ_MAX) return set_err(CSGPU_E_ARG, MANY_OBJ_CODE, objective);
  return many_clause_children(ck, d_slots, count, objective, d_children, stream);
}

extern "C" int csgpu_many_clause_checkpoint_fanout_obj(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                       int objective, const csgpu_many_start *d_owner_start,
                                                       const int64_t *d_offsets, csgpu_val *d_rows, int32_t *d_owner,
                                                       csgpu_many_start *d_start, int64_t total, void *stream) {
  if (objective != CS_OBJ_MIN && objective != CS_OBJ_MAX) return set_err(CSGPU_E_ARG, MANY_OBJ_CODE, objective);
  return many_clause_fanout(ck, d_slots, count, objective, d_owner_start, d_offsets, d_rows, d_owner, d_start, total, stream);
}

extern "C" uint64_t csgpu_many_best_key(int objective, int32_t best, uint32_t row) {
  return cs_many_best_key(objective_sense(objective), best, row);
}
extern "C" int csgpu_many_key_decode(int objective, uint64_t key, int32_t *best, uint32_t *row) {
  int32_t b = 0;
  uint32_t r = 0;
  const int found = cs_many_key_decode(objective_sense(objective), key, &b, &r);
  if (found && best != NULL) *best = b;
  if (found && row != NULL) *row = r;
  return found;
}

extern "C" int csgpu_many_fold_best(const csgpu_many_result *d_sub_results, const int32_t *d_sub_best, const int32_t *d_owner,
                                    int64_t total, int objective, uint64_t *d_key, void *stream) {
  if (d_sub_results == NULL || d_sub_best == NULL || d_owner == NULL || d_key == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (total < 0) return set_err(CSGPU_E_ARG, "negative record count");
  if (objective != CS_OBJ_MIN && objective != CS_OBJ_MAX)
    return set_err(CSGPU_E_ARG, "the best value is that of a MIN or a MAX walk (objective 2 or 3), not objective %d", objective);
  if (total >= 0x100000000ll) return set_err(CSGPU_E_LIMIT, "2^32 records or more in one call: a key names its row in 32 bits");
  if (total == 0) return CSGPU_OK;
  hipLaunchKernelGGL(cs_walk_fold_best, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const cs_dive_result *)d_sub_results, (const int *)d_sub_best, (const int *)d_owner, (long long)total,
                     objective_sense(objective), (unsigned long long *)d_key);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

/* ---- up to k solutions per instance of a clause model (cs_walk_upto): the ALL walk, left at the k-th solution, the rows
 * [count][max_solutions][n_vars] in d_solutions ---- */

/* the three entries: `pooled`, a call with a pool and slot numbers (else it has neither: the pool of capacity 0), and
 * `resume` (pooled, no roots) */
static int many_clauses_upto(const csgpu_model *m, const many_clauses_bufs *b, const csgpu_many_upto_options *options,
                             int pooled, int resume) {
  const int null_arg = m == NULL || (!resume && b->d_roots == NULL) || b->d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, b->count, null_arg ? 0 : options->max_nodes, pooled ? "slice" : "instance"))) return rc;
  if (options->max_solutions < 1)
    return set_err(CSGPU_E_ARG, "max_solutions must be at least 1: an instance stops at its k-th solution");
  if ((rc = many_clauses_check_model(m, CS_OBJ_ALL, b->count)) || (pooled && (rc = many_clauses_check_pool(m, b, MANY_POOL_WALK)))) return rc;
  cs_walk_ck wk = many_clauses_ck_arg(b, resume, CS_WALK_CK_UPTO);
  int upto = options->max_solutions;
  return many_clauses_launch(m, WALK_UPTO, m->host->n_vars, CS_OBJ_ALL, options->max_nodes, b, resume, &wk, &upto, NULL);
}

extern "C" int csgpu_solve_many_clauses_upto(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                             const csgpu_many_upto_options *options, csgpu_many_result *d_results,
                                             int32_t *d_solutions, void *stream) {
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions };
  return many_clauses_upto(m, &b, options, 0, 0);
}

extern "C" int csgpu_solve_many_clauses_upto_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                                          const csgpu_many_upto_options *options, csgpu_many_result *d_results,
                                                          int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                                          void *stream) {
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions, NULL /* no best */, ck, d_slots };
  return many_clauses_upto(m, &b, options, 1, 0);
}

extern "C" int csgpu_solve_many_clauses_upto_resume(const csgpu_model *m, int64_t count, const csgpu_many_upto_options *options,
                                                    csgpu_many_result *d_results, int32_t *d_solutions,
                                                    csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream) {
  const many_clauses_bufs b = { NULL, count, d_results, stream, d_solutions, NULL /* no best */, ck, d_slots };
  return many_clauses_upto(m, &b, options, 1, 1);
}

/* ---- Luby restarts with a seeded value order for ANY instances of a clause model (cs_walk_restart) ---- */

extern "C" int csgpu_solve_many_clauses_restarts(const csgpu_model *m, const csgpu_val *d_roots, const uint32_t *d_seeds,
                                                 int64_t count, const csgpu_many_restart_options *options,
                                                 csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_restarts,
                                                 void *stream) {
  const int null_arg = m == NULL || d_roots == NULL || d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "instance"))) return rc;
  if (options->restart_base < 0) return set_err(CSGPU_E_ARG, "restart_base must not be negative (0: no restarts)");
  if ((options->flags & ~CSGPU_MANY_ROTATE_FIRST) != 0) return set_err(CSGPU_E_ARG, "unknown flags 0x%x", (unsigned)options->flags);
  if ((rc = many_clauses_check_model(m, CS_OBJ_ANY, count))) return rc;
  cs_dive_rs dr;
  dr.seeds = d_seeds;
  dr.restarts = d_restarts;
  dr.restart_base = (long long)options->restart_base;
  dr.seed = options->seed;
  dr.flags = options->flags;
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions };
  return many_clauses_launch(m, WALK_RESTART, m->host->n_vars + 1 /* and the root node's */, CS_OBJ_ANY, options->max_nodes, &b, 0,
                             &dr, NULL, NULL);
}

/* ---- the engine's five variable orders and interval halving for the instances of a clause model (cs_walk_order) ---- */

/* what every ordered entry checks of its options, after csgpu_solve_many_clauses's own errors: the order, split_width,
 * `reserved`; *wo is then what the kernel takes */
static int many_clauses_ordered_options(const csgpu_many_order_options *options, int64_t *d_halvings, cs_walk_ord *wo) {
  if (options->order < 0 || options->order > 4)
    return set_err(CSGPU_E_ARG, "no variable order %d (0 none, 1 smallest domain, 2 largest domain, 3 smallest value, 4 largest value)",
                   (int)options->order);
  if (options->split_width < 0) return set_err(CSGPU_E_ARG, "split_width must not be negative (0: the engine's 256)");
  if (options->reserved != 0) return set_err(CSGPU_E_ARG, "reserved must be 0");
  wo->order = options->order;
  wo->split_width = options->split_width != 0 ? options->split_width : 256;
  wo->halvings = (long long *)d_halvings;
  return CSGPU_OK;
}

/* and what every ordered entry with a pool adds, last: the halving counts, the pool, its kind and its split_width */
static int many_clauses_ordered_pool(const csgpu_model *m, const many_clauses_bufs *b, const cs_walk_ord *wo) {
  int rc;
  if (wo->halvings == NULL)
    return set_err(CSGPU_E_ARG, "null argument: d_halvings, which a resumed instance's halving count goes on from");
  if ((rc = many_clauses_check_pool(m, b, MANY_POOL_ORDER))) return rc;
  if (b->ck->split_width != wo->split_width)
    return set_err(CSGPU_E_ARG, "the checkpoint pool was made for split_width %d, the call asks for %d: the frames of a slot differ",
                   b->ck->split_width, wo->split_width);
  return CSGPU_OK;
}

/* the three entries: the plain call, and with `pooled` the checkpointed call and its `resume` (no roots): cs_walk_order, or
 * cs_walk_order_resume on a pool of the ordered kind.  The checks, none of which touches the device, in the documented
 * order: csgpu_solve_many_clauses's own, this walk's three, then what a pooled call adds */
static int many_clauses_ordered(const csgpu_model *m, const many_clauses_bufs *b, const csgpu_many_order_options *options,
                                int64_t *d_halvings, int pooled, int resume) {
  const int null_arg = m == NULL || (!resume && b->d_roots == NULL) || b->d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, b->count, null_arg ? 0 : options->max_nodes, pooled ? "slice" : "instance")) ||
      (rc = many_clauses_check_model(m, options->objective, b->count)))
    return rc;
  /* after csgpu_solve_many_clauses's own errors, before any device call */
  cs_walk_ord wo;
  if ((rc = many_clauses_ordered_options(options, d_halvings, &wo))) return rc;
  if (!pooled)
    return many_clauses_launch(m, WALK_ORDER, (int)many_clauses_ordered_frames(m, options->split_width), options->objective,
                               options->max_nodes, b, 0, &wo, NULL, NULL);
  if ((rc = many_clauses_ordered_pool(m, b, &wo))) return rc;
  /* a checkpoint goes on under the objective and the order it was made under: another of either is another tree */
  cs_walk_ck wk = many_clauses_ck_arg(b, resume, options->objective | options->order << 3);
  return many_clauses_launch(m, WALK_ORDER_CK, b->ck->frames, options->objective, options->max_nodes, b, resume, &wk, &wo, NULL);
}

extern "C" int csgpu_solve_many_clauses_ordered(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                                const csgpu_many_order_options *options, csgpu_many_result *d_results,
                                                int32_t *d_solutions, int32_t *d_best, int64_t *d_halvings, void *stream) {
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions, d_best };
  return many_clauses_ordered(m, &b, options, d_halvings, 0, 0);
}

/* ---- the ordered walk in slices (cs_walk_order_resume): a pool whose slots have the frames of that walk ---- */

extern "C" size_t csgpu_many_clause_ordered_checkpoint_bytes(const csgpu_model *m, int32_t split_width) {
  if (m == NULL || split_width < 0 || !many_clauses_qualifies(m)) return 0;
  /* the header frame and the frames of a wave's stack (at most 33 n of them): 64 bits throughout */
  return ((size_t)many_clauses_ordered_frames(m, split_width) + 1) * ((size_t)m->host->n_vars + 1) * sizeof(cs_val);
}

extern "C" int csgpu_many_clause_ordered_checkpoints_create(const csgpu_model *m, int64_t capacity, int32_t split_width,
                                                            csgpu_many_checkpoints **out) {
  if (split_width < 0) return set_err(CSGPU_E_ARG, "split_width must not be negative (0: the engine's 256)");
  const int qualifies = csgpu_model_qualifies_many_clauses(m);
  return many_pool_create(m, capacity, MANY_POOL_ORDER, qualifies,
                          "model does not qualify for csgpu_solve_many_clauses (kernel 6 planned, its LDS slices fit a CU)",
                          csgpu_many_clause_ordered_checkpoint_bytes(m, split_width),
                          qualifies ? (int)many_clauses_ordered_frames(m, split_width) : 0, split_width != 0 ? split_width : 256, out);
}

extern "C" int csgpu_solve_many_clauses_ordered_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                                             const csgpu_many_order_options *options,
                                                             csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                                             int64_t *d_halvings, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                                             void *stream) {
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_clauses_ordered(m, &b, options, d_halvings, 1, 0);
}

extern "C" int csgpu_solve_many_clauses_ordered_resume(const csgpu_model *m, int64_t count, const csgpu_many_order_options *options,
                                                       csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                                       int64_t *d_halvings, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                                       void *stream) {
  const many_clauses_bufs b = { NULL, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_clauses_ordered(m, &b, options, d_halvings, 1, 1);
}

/* ---- the ordered walk from a start incumbent, and stopped ordered walks spread over the next launch (cs_walk_order_from;
 * cs_walk_order_children / cs_walk_order_fanout; cs_walk_fold_halvings) ---- */

/* the start call, checkpointed with a pool and slot numbers and plain with neither, and its resume (no roots, no starts),
 * which is checkpointed: cs_walk_order_from under MIN / MAX.  The checks, none of which touches the device, in the
 * documented order: csgpu_solve_many_clauses's own, the ordered walk's three, csgpu_solve_many_clauses_from's (the start,
 * the objective, the pool and the slots together), then what an ordered pool adds */
static int many_clauses_ordered_from(const csgpu_model *m, const many_clauses_bufs *b, const csgpu_many_start *d_start,
                                     const csgpu_many_order_options *options, int64_t *d_halvings, int resume) {
  const int null_arg = m == NULL || (!resume && b->d_roots == NULL) || b->d_results == NULL || options == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, b->count, null_arg ? 0 : options->max_nodes, resume ? "slice" : "instance")) ||
      (rc = many_clauses_check_model(m, options->objective, b->count)))
    return rc;
  cs_walk_ord wo;
  if ((rc = many_clauses_ordered_options(options, d_halvings, &wo))) return rc;
  if (!resume && d_start == NULL) return set_err(CSGPU_E_ARG, "null argument: d_start, the incumbents the instances start with");
  if (options->objective != CS_OBJ_MIN && options->objective != CS_OBJ_MAX)
    return set_err(CSGPU_E_ARG, "a start incumbent bounds a MIN / MAX walk (objective 2 or 3), not objective %d", options->objective);
  if ((b->ck == NULL) != (b->d_slots == NULL))
    return set_err(CSGPU_E_ARG, "null argument: a checkpointed call has a pool and slot numbers, a plain one neither");
  if (resume && b->ck == NULL) return set_err(CSGPU_E_ARG, "null argument: a checkpointed call has a pool and slot numbers");
  if (b->ck != NULL && (rc = many_clauses_ordered_pool(m, b, &wo))) return rc;
  const int frames = b->ck != NULL ? b->ck->frames : (int)many_clauses_ordered_frames(m, options->split_width);
  cs_walk_ck wk = many_clauses_ck_arg(b, resume, options->objective | options->order << 3);
  const cs_walk_start *starts = (const cs_walk_start *)d_start;
  return many_clauses_launch(m, WALK_ORDER_FROM, frames, options->objective, options->max_nodes, b, resume, &wk, &wo, &starts);
}

extern "C" int csgpu_solve_many_clauses_ordered_from(const csgpu_model *m, const csgpu_val *d_roots, const csgpu_many_start *d_start,
                                                     int64_t count, const csgpu_many_order_options *options,
                                                     csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                                     int64_t *d_halvings, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                                     void *stream) {
  const many_clauses_bufs b = { d_roots, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_clauses_ordered_from(m, &b, d_start, options, d_halvings, 0);
}

extern "C" int csgpu_solve_many_clauses_ordered_from_resume(const csgpu_model *m, int64_t count,
                                                            const csgpu_many_order_options *options, csgpu_many_result *d_results,
                                                            int32_t *d_solutions, int32_t *d_best, int64_t *d_halvings,
                                                            csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream) {
  const many_clauses_bufs b = { NULL, count, d_results, stream, d_solutions, d_best, ck, d_slots };
  return many_clauses_ordered_from(m, &b, NULL, options, d_halvings, 1);
}

/* what the count and the fan-out of an ordered pool check alike, after their null arguments and counts: the objective, the
 * order, the kind of the pool, the number of instances */
static int many_clause_ordered_fan_check(const csgpu_many_checkpoints *ck, int64_t count, int objective, int order) {
  if (objective != CS_OBJ_ALL && objective != CS_OBJ_MIN && objective != CS_OBJ_MAX)
    return set_err(CSGPU_E_ARG, "the checkpoints of an ALL, a MIN or a MAX walk are asked for (objective 1, 2 or 3), not objective %d",
                   objective);
  if (order < 0 || order > 4)
    return set_err(CSGPU_E_ARG, "no variable order %d (0 none, 1 smallest domain, 2 largest domain, 3 smallest value, 4 largest value)",
                   order);
  if (ck->kind != MANY_POOL_ORDER) return set_err(CSGPU_E_ARG, MANY_POOL_KIND_ORDER);
  if (count > 0x7fffffff) return set_err(CSGPU_E_LIMIT, MANY_FAN_LIMIT);
  return CSGPU_OK;
}

extern "C" int csgpu_many_clause_ordered_checkpoint_children(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                             int objective, int order, int64_t *d_children, int32_t *d_unsplit,
                                                             void *stream) {
  if (ck == NULL || d_slots == NULL || d_children == NULL || d_unsplit == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (count < 0) return set_err(CSGPU_E_ARG, "negative instance count");
  int rc;
  if ((rc = many_clause_ordered_fan_check(ck, count, objective, order))) return rc;
  if (count == 0) return CSGPU_OK;
  const csgpu_model *m = ck->m;
  const unsigned grid = (unsigned)((count + CS_DIVE_FAN_WAVES - 1) / CS_DIVE_FAN_WAVES);
  hipLaunchKernelGGL(cs_walk_order_children, dim3(grid), dim3(CS_DIVE_FAN_WAVES * CS_WAVE), 0, (hipStream_t)stream,
                     m->host->n_vars, ck->frames, ck->split_width, (const cs_val *)m->d_walk_root, (const cs_val *)ck->d_pool,
                     (int)ck->capacity, (const int *)d_slots, (long long)count, (long long *)d_children, (int *)d_unsplit,
                     objective | order << 3);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_many_clause_ordered_checkpoint_fanout(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                           int objective, int order, const csgpu_many_start *d_owner_start,
                                                           const int64_t *d_offsets, csgpu_val *d_rows, int32_t *d_owner,
                                                           csgpu_many_start *d_start, int64_t total, void *stream) {
  if (ck == NULL || d_slots == NULL || d_offsets == NULL || d_rows == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (count < 0) return set_err(CSGPU_E_ARG, "negative instance count");
  if (total < 0) return set_err(CSGPU_E_ARG, "negative row count");
  int rc;
  if ((rc = many_clause_ordered_fan_check(ck, count, objective, order))) return rc;
  if (objective == CS_OBJ_ALL && (d_owner_start != NULL || d_start != NULL))
    return set_err(CSGPU_E_ARG, "start incumbents travel with objective MIN / MAX: d_owner_start and d_start are NULL under ALL");
  if (objective != CS_OBJ_ALL && d_start == NULL)
    return set_err(CSGPU_E_ARG, "null argument: d_start, where the start incumbent of every row goes under MIN / MAX");
  if (count == 0 || total == 0) return CSGPU_OK;
  const csgpu_model *m = ck->m;
  const unsigned grid = (unsigned)((count + CS_DIVE_FAN_WAVES - 1) / CS_DIVE_FAN_WAVES);
  hipLaunchKernelGGL(cs_walk_order_fanout, dim3(grid), dim3(CS_DIVE_FAN_WAVES * CS_WAVE), 0, (hipStream_t)stream, m->host->n_vars,
                     ck->frames, ck->split_width, (const cs_val *)m->d_walk_root, (const cs_val *)ck->d_pool, (int)ck->capacity,
                     (const int *)d_slots, (long long)count, (const long long *)d_offsets, (long long)total, (cs_val *)d_rows,
                     (int *)d_owner, objective | order << 3, (const cs_walk_start *)d_owner_start, (cs_walk_start *)d_start);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_many_fold_halvings(const int64_t *d_sub_halvings, const int32_t *d_owner, int64_t total, int64_t *d_halvings,
                                        void *stream) {
  if (d_sub_halvings == NULL || d_owner == NULL || d_halvings == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (total < 0) return set_err(CSGPU_E_ARG, "negative record count");
  if (total > 256ll * 0x7fffffff) return set_err(CSGPU_E_LIMIT, "more than 2^39 - 256 records in one call");
  if (total == 0) return CSGPU_OK;
  hipLaunchKernelGGL(cs_walk_fold_halvings, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const long long *)d_sub_halvings, (const int *)d_owner, (long long)total, (long long *)d_halvings);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

/* ---- every solution of every instance of a clause model under ALL, through one bounded stream (cs_walk_stream) ---- */

extern "C" int csgpu_solve_many_clauses_stream(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                               const csgpu_many_options *options, csgpu_many_result *d_results,
                                               csgpu_many_checkpoints *ck, int32_t *d_slots, const csgpu_many_stream *out,
                                               void *stream) {
  const int null_arg = m == NULL || d_roots == NULL || d_results == NULL || options == NULL || ck == NULL || d_slots == NULL || out == NULL;
  int rc;
  if ((rc = many_check_head(null_arg, count, null_arg ? 0 : options->max_nodes, "slice"))) return rc;
  /* before the model is looked at: ALL only, and a stream that can take a row */
  if (options->objective != CS_OBJ_ALL)
    return set_err(CSGPU_E_ARG, "csgpu_solve_many_clauses_stream walks under ALL (objective 1), not objective %d", options->objective);
  if (out->capacity < 1)
    return set_err(CSGPU_E_ARG, "the solution stream has room for at least one row (capacity %lld)", (long long)out->capacity);
  if (out->d_rows == NULL || out->d_owner == NULL || out->d_count == NULL) return set_err(CSGPU_E_ARG, "null pointer in the solution stream");
  many_clauses_bufs b = { d_roots, count, d_results, stream }; /* no rows of its own: they go to *out */
  b.ck = ck;
  b.d_slots = d_slots;
  if ((rc = many_clauses_check_model(m, CS_OBJ_ALL, count)) || (rc = many_clauses_check_pool(m, &b, MANY_POOL_WALK))) return rc;
  /* not a resume: d_slots says per instance whether it starts or goes on, so the workspace is a fresh call's */
  cs_walk_ck wk = many_clauses_ck_arg(&b, 0, CS_WALK_CK_STREAM);
  cs_dive_out ok;
  ok.rows = out->d_rows;
  ok.owner = out->d_owner;
  ok.count = (unsigned long long *)out->d_count;
  ok.capacity = (long long)out->capacity;
  return many_clauses_launch(m, WALK_STREAM, m->host->n_vars, CS_OBJ_ALL, options->max_nodes, &b, 0, &wk, &ok, NULL);
}

#ifdef CS_SHAVE_TIMELINE
extern "C" int csgpu_debug_shave_timeline(unsigned long long *out, int waves) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(cs_shave_tl), (size_t)waves * 3 * sizeof(unsigned long long)));
  return CSGPU_OK;
}
#endif

extern "C" int csgpu_propagate_batch_fb(const csgpu_model *m, const csgpu_val *d_states_in, const uint64_t *d_forb_in,
                                        const csgpu_node *d_nodes, csgpu_val *d_states_out, uint64_t *d_forb_out,
                                        csgpu_result *d_results, int64_t batch, void *stream) {
  return csgpu_internal_propagate_fb(m, d_states_in, d_forb_in, d_nodes, d_states_out, d_forb_out, d_results, batch, NULL,
                                     stream);
}

/* batch = upper bound the launch is sized for; d_batch (nullable) = the real count, on the device */
extern "C" int csgpu_internal_propagate_fb(const csgpu_model *m, const csgpu_val *d_states_in, const uint64_t *d_forb_in,
                                           const csgpu_node *d_nodes, csgpu_val *d_states_out, uint64_t *d_forb_out,
                                           csgpu_result *d_results, int64_t batch, const uint64_t *d_batch,
                                           void *stream) {
  if (m == NULL || batch < 0) return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (!kernel_qualifies(m, 3)) return set_err(CSGPU_E_LIMIT, "model does not qualify for the forbidden-set kernel");
  if (batch == 0) return CSGPU_OK;
  if (d_states_in == NULL || d_nodes == NULL || d_states_out == NULL || d_results == NULL)
    return set_err(CSGPU_E_ARG, "null argument");
  if (kernel_qualifies(m, 4) && m->kernel_choice != 3)
    return launch_regs(m, d_states_in, d_forb_in, d_nodes, d_states_out, d_forb_out, d_results, batch, d_batch, 0, 0, stream);
  const cs_planned *k = &m->plan.bitset;
  /* nodes per wave at a time: CS_CHUNK for large batches (one coalesced record load per 16 nodes); a batch
   * smaller than the machine is spread thinner so that it does not run 16 nodes deep on a few waves */
  int csz = shrink_chunk(CS_CHUNK, batch, (int64_t)m->n_cus * 32);
  const int64_t chunks = (batch + csz - 1) / csz;
  int64_t grid = (int64_t)m->n_cus * (int64_t)k->per_cu;
  const int64_t need = (chunks + k->waves - 1) / k->waves;
  if (grid > need) grid = need;
  cs_tables tab = m->tab;
  tab.adj_off = m->d_sym_off; /* the symmetric lists */
  const void *packed = m->d_sym_packed;
  int n_adj = m->img->sym_n_adj, obits = m->img->sym_obits, dmin = m->img->sym_dmin;
  const int *root_lo = m->d_root_lo;
  long long nb = (long long)batch;
  void *args[] = { &tab, &packed, &n_adj, &obits, &dmin, &root_lo, &d_states_in, &d_forb_in, &d_nodes,
                   &d_states_out, &d_forb_out, &d_results, &nb, &d_batch, &csz };
  HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)grid), dim3((unsigned)(k->waves * CS_WAVE)), args, k->lds, (hipStream_t)stream));
  return CSGPU_OK;
}

/* ---- sets-only states (include/csolve_gpu.h) ------------------------------------------------------------ */

__global__ void cs_fill_identity_nodes(cs_node_in *nodes, long long count) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    cs_node_in nd;
    nd.var = -1; nd.lo = 0; nd.hi = 0; nd.parent = (int)i;
    nodes[i] = nd;
  }
}

static int sets_ready(const csgpu_model *m) {
  if (m == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (!kernel_qualifies(m, 4)) return set_err(CSGPU_E_LIMIT, "model does not qualify for the register-resident forbidden-set kernel");
  return CSGPU_OK;
}

extern "C" int csgpu_sets_pack(const csgpu_model *m, const csgpu_val *d_states, uint64_t *d_sets, int64_t count, void *stream) {
  int rc = sets_ready(m);
  if (rc != CSGPU_OK) return rc;
  if (count < 0) return set_err(CSGPU_E_ARG, "bad argument");
  if (count == 0) return CSGPU_OK;
  if (d_states == NULL || d_sets == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (count > 0x7fffffff) return set_err(CSGPU_E_LIMIT, "too many states");
  cs_node_in *d_nodes = NULL;
  cs_node_out *d_res = NULL;
  HIP_TRY(hipMalloc((void **)&d_nodes, (size_t)count * sizeof(cs_node_in)));
  if (hipMalloc((void **)&d_res, (size_t)count * sizeof(cs_node_out)) != hipSuccess) {
    (void)hipFree(d_nodes);
    return set_err(CSGPU_E_HIP, "out of device memory");
  }
  hipLaunchKernelGGL(cs_fill_identity_nodes, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_nodes, (long long)count);
  /* rebuild mode (every valued variable pushes), the intervals folded into the sets on the way out */
  rc = launch_regs(m, d_states, NULL, (const csgpu_node *)d_nodes, NULL, d_sets, (csgpu_result *)d_res, count, NULL, 0,
                   CS_K4_OUT_RESTRICT, stream);
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(d_nodes);
  (void)hipFree(d_res);
  if (rc != CSGPU_OK) return rc;
  if (e != hipSuccess) return set_err(CSGPU_E_HIP, "%s", hipGetErrorString(e));
  return CSGPU_OK;
}

extern "C" int csgpu_sets_unpack(const csgpu_model *m, const uint64_t *d_sets, csgpu_val *d_states, int64_t count, void *stream) {
  int rc = sets_ready(m);
  if (rc != CSGPU_OK) return rc;
  if (count < 0) return set_err(CSGPU_E_ARG, "bad argument");
  if (count == 0) return CSGPU_OK;
  if (d_states == NULL || d_sets == NULL) return set_err(CSGPU_E_ARG, "null argument");
  const int n = m->host->n_vars;
  int64_t blocks = (count * n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  const unsigned long long *sets = (const unsigned long long *)d_sets;
  cs_val *states = (cs_val *)d_states;
  switch (m->fb_words) {
  case 1: hipLaunchKernelGGL(cs_sets_unpack<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, m->d_root_lo, sets, states, (long long)count); break;
  case 2: hipLaunchKernelGGL(cs_sets_unpack<2>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, m->d_root_lo, sets, states, (long long)count); break;
  default: hipLaunchKernelGGL(cs_sets_unpack<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, m->d_root_lo, sets, states, (long long)count); break;
  }
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_propagate_batch_sets(const csgpu_model *m, const uint64_t *d_sets_in, const csgpu_node *d_nodes,
                                          uint64_t *d_sets_out, csgpu_result *d_results, int64_t batch, void *stream) {
  int rc = sets_ready(m);
  if (rc != CSGPU_OK) return rc;
  if (batch < 0) return set_err(CSGPU_E_ARG, "bad argument");
  if (batch == 0) return CSGPU_OK;
  if (d_sets_in == NULL || d_nodes == NULL || d_sets_out == NULL || d_results == NULL)
    return set_err(CSGPU_E_ARG, "null argument");
  return launch_regs(m, NULL, d_sets_in, d_nodes, NULL, d_sets_out, d_results, batch, NULL, 1, 0, stream);
}

extern "C" int csgpu_model_get_kernel(const csgpu_model *m) {
  if (m == NULL) return CSGPU_E_ARG;
  if (m->kernel_choice) return m->kernel_choice;
  /* pure != networks: the forbidden-set kernels, the sets rebuilt from the incoming state when the caller
   * carries none (queens-64, 2^18 nodes: 0.14 ms against 0.51 ms of kernel 2; queens-16: 0.06 against 0.51) */
  if (kernel_qualifies(m, 3)) {
    /* no sets passed: small models several nodes per wave with the sets rebuilt (5), otherwise the
     * interval-only shaving kernel (7), which needs no sets at all */
    if (kernel_qualifies(m, 4)) return kernel_qualifies(m, 5) ? 5 : 7;
    /* more than 256 variables and no sets to inherit: rebuilding them costs one list scan per VALUED variable of
     * the incoming state (sudoku-25, 2^18 nodes: 6.2 ms), the event-driven kernels scan one list per narrowing
     * (kernel 2: 1.16 ms, kernel 1: 1.18 ms).  Callers that carry the sets use csgpu_propagate_batch_fb (kernel 3:
     * 0.91 ms on that batch). */
    return kernel_qualifies(m, 2) ? 2 : 1;
  }
  if (kernel_qualifies(m, 2)) return 2;
  /* 8 clauses per lane: kernel 6 for small batches only, see csgpu_internal_propagate_objdev */
  return kernel_qualifies(m, 6) && m->plan.rounds_cpl <= 4 ? 6 : 1;
}

/* ---- batched propagation ----------------------------------------------------------- */

extern "C" int csgpu_propagate_batch(const csgpu_model *m, const csgpu_val *d_states_in, const csgpu_node *d_nodes,
                                     csgpu_val *d_states_out, csgpu_result *d_results, int64_t batch, void *stream) {
  return csgpu_propagate_batch_obj(m, d_states_in, d_nodes, d_states_out, d_results, batch, CS_DOM_MIN, CS_DOM_MAX,
                                   stream);
}

extern "C" int csgpu_propagate_batch_obj(const csgpu_model *m, const csgpu_val *d_states_in, const csgpu_node *d_nodes,
                                         csgpu_val *d_states_out, csgpu_result *d_results, int64_t batch,
                                         int32_t obj_lo, int32_t obj_hi, void *stream) {
  return csgpu_internal_propagate_obj(m, d_states_in, d_nodes, d_states_out, d_results, batch, NULL, obj_lo, obj_hi, stream);
}

extern "C" int csgpu_internal_propagate_obj(const csgpu_model *m, const csgpu_val *d_states_in, const csgpu_node *d_nodes,
                                            csgpu_val *d_states_out, csgpu_result *d_results, int64_t batch,
                                            const uint64_t *d_batch, int32_t obj_lo, int32_t obj_hi, void *stream) {
  return csgpu_internal_propagate_objdev(m, d_states_in, d_nodes, d_states_out, d_results, batch, d_batch, obj_lo, obj_hi,
                                         NULL, 0, stream);
}

/* d_best (nullable) / sense: the incumbent is read from device memory when the kernel starts */
extern "C" int csgpu_internal_propagate_objdev(const csgpu_model *m, const csgpu_val *d_states_in,
                                               const csgpu_node *d_nodes, csgpu_val *d_states_out,
                                               csgpu_result *d_results, int64_t batch, const uint64_t *d_batch,
                                               int32_t obj_lo, int32_t obj_hi, const int32_t *d_best, int sense,
                                               void *stream) {
  if (m == NULL || batch < 0) return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (batch == 0) return CSGPU_OK; /* an empty batch needs no buffers */
  if (d_states_in == NULL || d_nodes == NULL || d_states_out == NULL || d_results == NULL)
    return set_err(CSGPU_E_ARG, "null argument");
  hipStream_t s = (hipStream_t)stream;
  const cs_val *in = (const cs_val *)d_states_in;
  const cs_node_in *nodes = (const cs_node_in *)d_nodes;
  cs_val *out = (cs_val *)d_states_out;
  cs_node_out *res = (cs_node_out *)d_results;
  cs_tables tab = m->tab;
  if (m->host->obj_var >= 0 && (obj_lo != CS_DOM_MIN || obj_hi != CS_DOM_MAX || (d_best != NULL && sense != 0))) {
    tab.obj_var = m->host->obj_var;
    tab.obj_lo = obj_lo;
    tab.obj_hi = obj_hi;
    if (d_best != NULL && sense != 0) {
      tab.obj_best_dev = d_best;
      tab.obj_sense = sense;
    }
  }
  const int kernel = csgpu_model_get_kernel(m);
  if (kernel == 7 && tab.obj_var < 0)
    return launch_shave(m, d_states_in, d_nodes, d_states_out, d_results, batch, d_batch, stream);
  if (kernel >= 3 && kernel <= 5 && tab.obj_var < 0)
    return csgpu_internal_propagate_fb(m, d_states_in, NULL, d_nodes, d_states_out, NULL, d_results, batch, d_batch, stream);
  const unsigned long long *bdev = (const unsigned long long *)d_batch;
  long long nb = (long long)batch;
  if (kernel == 2 && tab.obj_var < 0 && d_batch == NULL) {
    const cs_planned *k = &m->plan.lds;
    /* persistent workgroups: as many as stay resident */
    int64_t grid = (int64_t)m->n_cus * (int64_t)k->per_cu;
    /* nodes a wave takes at a time: 16 when every wave gets several such chunks, fewer for smaller batches (a wave
     * with two chunks next to one with one is a launch twice as long as it needs to be) */
    int csz = (int)(batch / (grid * k->waves * 4));
    csz = csz < 1 ? 1 : (csz > CS_CHUNK ? CS_CHUNK : csz);
    if (m->k2_csz) csz = m->k2_csz;
    const int64_t chunks = (batch + csz - 1) / csz;
    const int64_t need = (chunks + k->waves - 1) / k->waves;
    if (grid > need) grid = need;
    int n_adj = m->img->n_adj, obits = m->img->packed_obits, dmin = m->img->packed_dmin;
    const void *packed = m->d_adj_packed;
    void *args[] = { &tab, &packed, &n_adj, &obits, &dmin, &in, &nodes, &out, &res, &nb, &csz };
    HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)grid), dim3((unsigned)(k->waves * CS_WAVE)), args, k->lds, s));
    return CSGPU_OK;
  }
  /* kernel 6 when asked for; automatically for models of at most 256 clauses (faster at every batch size
   * measured), and with 257-512 clauses for small batches only (lower latency, 14 us against 21 us per launch
   * on schedule-20, but less throughput: 215 us against 122 us for 65,536 nodes) -- the search engine's
   * device-counted batches are small by construction */
  const int use6 = kernel == 6 || (m->kernel_choice == 0 && kernel == 1 && !kernel_qualifies(m, 3) && kernel_qualifies(m, 6) &&
                                   (d_batch != NULL || batch <= 8192));
  const cs_planned *k = use6 ? &m->plan.rounds : &m->plan.events;
  /* enough workgroups to fill the chip several times over, the rest by grid stride */
  int64_t blocks = (batch + CS_WAVES_PER_BLOCK - 1) / CS_WAVES_PER_BLOCK;
  if (blocks > (int64_t)m->n_cus * k->per_cu * 4) blocks = (int64_t)m->n_cus * k->per_cu * 4;
  void *args[] = { &tab, &in, &nodes, &out, &res, &nb, &bdev };
  HIP_TRY(hipLaunchKernel(k->fn, dim3((unsigned)blocks), dim3(CS_BLOCK), args, k->lds, s));
  return CSGPU_OK;
}

/* one wave per state while four domain arrays fit 64 KB of LDS, else one workgroup per state */
static int launch_eval_root(const csgpu_model *m, const csgpu_val *d_states, const int32_t *d_list, const uint64_t *d_count,
                            int64_t count, int32_t *d_truth, void *stream) {
  const size_t row = (size_t)m->host->n_vars * sizeof(cs_val);
  if (row * CS_WAVES_PER_BLOCK <= 64u * 1024u) {
    /* grid-stride: enough workgroups to fill the machine, every wave keeps its share of the clause table */
    int64_t blocks = (count + CS_WAVES_PER_BLOCK - 1) / CS_WAVES_PER_BLOCK;
    if (blocks > (int64_t)m->n_cus * 16) blocks = (int64_t)m->n_cus * 16;
    /* a count that stays on the device is the handful of complete children of a search iteration, `count` only their
     * bound: one workgroup per CU (the waves stride over more), not thousands that start to find nothing to do */
    if (d_count != NULL && blocks > (int64_t)m->n_cus) blocks = (int64_t)m->n_cus;
    const int per = (m->img->n_clauses + CS_WAVE - 1) / CS_WAVE;
#define CS_LAUNCH_EVAL_T(CPL, TREE)                                                                \
  hipLaunchKernelGGL((cs_eval_root_waves<CPL, TREE>), dim3((unsigned)blocks), dim3(CS_BLOCK), row * CS_WAVES_PER_BLOCK, \
                     (hipStream_t)stream, m->tab, (const cs_val *)d_states, d_truth, (const int *)d_list,                \
                     (const unsigned long long *)d_count, (long long)count)
#define CS_LAUNCH_EVAL(CPL)                                                                        \
  do {                                                                                             \
    if (m->img->n_trees > 0) CS_LAUNCH_EVAL_T(CPL, true);                                          \
    else CS_LAUNCH_EVAL_T(CPL, false);                                                             \
  } while (0)
    if (per <= 1) CS_LAUNCH_EVAL(1);
    else if (per <= 2) CS_LAUNCH_EVAL(2);
    else if (per <= 4) CS_LAUNCH_EVAL(4);
    else if (per <= 8) CS_LAUNCH_EVAL(8);
    else CS_LAUNCH_EVAL(0);
#undef CS_LAUNCH_EVAL
#undef CS_LAUNCH_EVAL_T
  } else {
    hipLaunchKernelGGL(cs_eval_root, dim3((unsigned)count), dim3(CS_BLOCK), row + 16, (hipStream_t)stream, m->tab,
                       (const cs_val *)d_states, d_truth, (const int *)d_list, (const unsigned long long *)d_count);
  }
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

extern "C" int csgpu_eval_batch(const csgpu_model *m, const csgpu_val *d_states, int32_t *d_truth, int64_t batch,
                                void *stream) {
  if (m == NULL || d_states == NULL || d_truth == NULL || batch < 0) return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (batch == 0) return CSGPU_OK;
  if (batch > 0x7fffffff) return set_err(CSGPU_E_LIMIT, "batch too large");
  return launch_eval_root(m, d_states, NULL, NULL, batch, d_truth, stream);
}

/* instance i = row d_list[i] of d_states, i < *d_count <= bound (the count stays on the device) */
extern "C" int csgpu_internal_eval_list(const csgpu_model *m, const csgpu_val *d_states, const int32_t *d_list,
                                        const uint64_t *d_count, int64_t bound, int32_t *d_truth, void *stream) {
  if (m == NULL || d_states == NULL || d_list == NULL || d_count == NULL || d_truth == NULL || bound < 0)
    return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (bound == 0) return CSGPU_OK;
  if (bound > 0x7fffffff) return set_err(CSGPU_E_LIMIT, "batch too large");
  return launch_eval_root(m, d_states, d_list, d_count, bound, d_truth, stream);
}

extern "C" int csgpu_eval_clauses(const csgpu_model *m, const csgpu_val *d_state, csgpu_val *d_vals, void *stream) {
  if (m == NULL || d_state == NULL || d_vals == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (m->host->n_clauses == 0) return CSGPU_OK;
  const size_t lds = (size_t)m->host->n_vars * sizeof(cs_val) + 16;
  unsigned blocks = (unsigned)((m->host->n_clauses + CS_BLOCK - 1) / CS_BLOCK);
  if (blocks > 1024u) blocks = 1024u;
  hipLaunchKernelGGL(cs_eval_clauses, dim3(blocks), dim3(CS_BLOCK), lds, (hipStream_t)stream, m->tab,
                     (const cs_val *)d_state, (cs_val *)d_vals);
  HIP_TRY(hipGetLastError());
  return CSGPU_OK;
}

/* `count` values of one variable on one parent state, host buffers: the sibling batch of the drop-in shim (the
 * driver tries them one after the other, csolve.c:331-338; the device takes them at once).  The parent, the node
 * records, the results and the new states live in mapped pinned memory: one launch, one wait. */
extern "C" int csgpu_propagate_values(const csgpu_model *cm, const csgpu_val *state, int32_t var, const int32_t *values,
                                      int32_t count, csgpu_val *states_out, csgpu_result *results) {
  csgpu_model *m = (csgpu_model *)cm;
  if (m == NULL || state == NULL || values == NULL || states_out == NULL || results == NULL)
    return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  const int n = m->host->n_vars;
  if (var < 0 || var >= n || count < 0 || count > (1 << 20)) return set_err(CSGPU_E_ARG, "bad argument");
  if (count == 0) return CSGPU_OK;
  const size_t row = (size_t)n * sizeof(cs_val);
  const size_t off_nodes = (row + 255) & ~(size_t)255;
  const size_t off_res = off_nodes + (((size_t)count * sizeof(cs_node_in) + 255) & ~(size_t)255);
  const size_t off_out = off_res + (((size_t)count * sizeof(cs_node_out) + 255) & ~(size_t)255);
  const size_t need = off_out + (size_t)count * row;
  if (need > m->values_cap) {
    if (m->h_values != NULL) (void)hipHostFree(m->h_values);
    m->h_values = NULL;
    m->values_cap = 0;
    HIP_TRY(hipHostMalloc((void **)&m->h_values, need * 2, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer((void **)&m->d_values, m->h_values, 0));
    m->values_cap = need * 2;
  }
  memcpy(m->h_values, state, row);
  cs_node_in *nd = (cs_node_in *)(m->h_values + off_nodes);
  for (int32_t i = 0; i < count; i++) { nd[i].var = var; nd[i].lo = nd[i].hi = values[i]; nd[i].parent = 0; }
  int rc = csgpu_propagate_batch(m, (const csgpu_val *)m->d_values, (const csgpu_node *)(m->d_values + off_nodes),
                                 (csgpu_val *)(m->d_values + off_out), (csgpu_result *)(m->d_values + off_res), count, NULL);
  if (rc != CSGPU_OK) return rc;
  { const int rcw = wait_null_stream(); if (rcw != CSGPU_OK) return rcw; }
  memcpy(results, m->h_values + off_res, (size_t)count * sizeof *results);
  memcpy(states_out, m->h_values + off_out, (size_t)count * row);
  return CSGPU_OK;
}

/* One node with its trail.  The general kernel (one wave) records every narrowing with the clause that made
 * it -- what the reference's bind() keeps as binding_t.clause (csolve.h:73-79) and its conflict analysis walks
 * (conflict.c:290-316) -- and the point of failure. */
extern "C" int csgpu_propagate_one_traced(const csgpu_model *cm, const csgpu_val *state, csgpu_node node,
                                          csgpu_val *state_out, csgpu_result *result, int32_t *trace, int32_t cap,
                                          int32_t *count) {
  csgpu_model *m = const_cast<csgpu_model *>(cm);
  if (m == NULL || state == NULL || state_out == NULL || result == NULL || trace == NULL || cap < 1 || count == NULL)
    return set_err(CSGPU_E_ARG, "bad argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (m->d_adj_clause == NULL) {
    int rc = upload(m->img->adj_clause, (size_t)(m->img->n_adj ? m->img->n_adj : 1) * 4, &m->d_adj_clause);
    if (rc != CSGPU_OK) return rc;
  }
  if (m->trace_cap < cap) {
    if (m->h_trace != NULL) (void)hipHostFree(m->h_trace);
    m->h_trace = NULL;
    HIP_TRY(hipHostMalloc((void **)&m->h_trace, (size_t)cap * 16 + 16, hipHostMallocMapped));
    m->h_trace_n = (unsigned *)(m->h_trace + (size_t)cap * 4);
    m->trace_cap = cap;
  }
  const size_t nbytes = (size_t)m->host->n_vars * sizeof(cs_val);
  const size_t part = (nbytes + 63) & ~(size_t)63;
  node.parent = 0;
  memcpy(m->h_one, state, nbytes);
  memcpy(m->h_one + part, &node, sizeof node);
  *m->h_trace_n = 0u;
  cs_tables tab = m->tab;
  tab.adj_clause = m->d_adj_clause;
  void *dev = NULL;
  HIP_TRY(hipHostGetDevicePointer(&dev, m->h_trace, 0));
  tab.trace_log = (int4 *)dev;
  tab.trace_n = (unsigned *)((int32_t *)dev + (size_t)m->trace_cap * 4); /* where h_trace_n points */
  tab.trace_cap = (unsigned)cap;
  const cs_val *in = m->d_one_in;
  const cs_node_in *nd = m->d_one_node;
  cs_val *out = m->d_one_out;
  cs_node_out *res = m->d_one_res;
  long long one = 1;
  const unsigned long long *no_count = NULL;
  void *args[] = { &tab, &in, &nd, &out, &res, &one, &no_count };
  HIP_TRY(hipLaunchKernel(m->plan.traced.fn, dim3(1), dim3(CS_BLOCK), args, m->plan.traced.lds, (hipStream_t)NULL));
  { const int rcw = wait_null_stream(); if (rcw != CSGPU_OK) return rcw; }
  memcpy(result, m->h_one + part + 64, sizeof *result);
  if (result->status >= 0) memcpy(state_out, m->h_one + part + 128, nbytes);
  const unsigned n = *m->h_trace_n;
  *count = (int32_t)n;
  memcpy(trace, m->h_trace, (size_t)(n < (unsigned)cap ? n : (unsigned)cap) * 16);
  return CSGPU_OK;
}

/* One node of a pure != network with its trail as causes: kernel 7's tracing variant, one wave. */
static double srv_now(void) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static cs_mailbox_head *srv_box(const csgpu_model *m) { return (cs_mailbox_head *)m->h_box; }

/* does this model use the server?  (kernel 7's models whose table leaves room for the trail in LDS) */
static int server_usable(csgpu_model *m) {
  if (m->srv_off) return 0;
  if (m->h_box != NULL) return 1;
  const char *e = getenv("CSGPU_SERVER");
  if ((e != NULL && e[0] == '0') || m->plan.server.fn == NULL) { m->srv_off = 1; return 0; }
  const size_t nbytes = ((size_t)m->host->n_vars * sizeof(cs_val) + 63) & ~(size_t)63;
  m->box_state_off = (sizeof(cs_mailbox_head) + 63) & ~(size_t)63;
  m->box_out_off = m->box_state_off + nbytes;
  m->box_trace_off = m->box_out_off + nbytes;
  const size_t total = m->box_trace_off + (size_t)CS_SHAVE_TRACE_LDS * 16;
  if (hipHostMalloc((void **)&m->h_box, total, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipStreamCreateWithFlags(&m->srv_stream, hipStreamNonBlocking) != hipSuccess ||
      hipFuncSetAttribute(m->plan.server.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)m->plan.server.lds) != hipSuccess) {
    (void)hipGetLastError();
    if (m->h_box != NULL) (void)hipHostFree(m->h_box);
    m->h_box = NULL;
    m->srv_off = 1;
    return 0;
  }
  memset(m->h_box, 0, total);
  m->srv_seq = 0;
  for (int i = 0; i < 16; i++)
    if (g_srv_models[i] == NULL) { g_srv_models[i] = m; break; }
  return 1;
}

/* start a resident wave (none is alive) and wait until it says so */
static int server_start(csgpu_model *m) {
  cs_mailbox_head *box = srv_box(m);
  if (m->srv_launched) server_reap(m); /* the previous one has left (alive == 0): reap it */
  void *dev = NULL;
  HIP_TRY(hipHostGetDevicePointer(&dev, m->h_box, 0));
  cs_mailbox_head *d_box = (cs_mailbox_head *)dev;
  unsigned long long *d_in = (unsigned long long *)((unsigned char *)dev + m->box_state_off);
  unsigned long long *d_out = (unsigned long long *)((unsigned char *)dev + m->box_out_off);
  int4 *d_trace = (int4 *)((unsigned char *)dev + m->box_trace_off);
  int n = m->host->n_vars, slots = m->img->dense_slots, dmin_d = m->img->dense_dmin;
  const void *tab_d = m->d_dense_tab;
  const int *root_lo_d = m->d_root_lo, *sym_off = m->d_sym_off;
  unsigned cap = CS_SHAVE_TRACE_LDS;
  unsigned long long idle = 200000ull; /* 2 ms of the 100 MHz clock: a search calls every few microseconds */
  { const char *e = getenv("CSGPU_SERVER_IDLE_US"); if (e != NULL && atoll(e) > 0) idle = (unsigned long long)atoll(e) * 100ull; }
  void *args[] = { &n, &tab_d, &slots, &dmin_d, &root_lo_d, &sym_off, &d_box, &d_in, &d_out, &d_trace, &cap, &idle };
  const cs_planned *k = &m->plan.server;
  HIP_TRY(hipLaunchKernel(k->fn, dim3(1), dim3((unsigned)(k->waves * CS_WAVE)), args, k->lds, m->srv_stream));
  m->srv_launched = 1;
  m->srv_starts++;
  const double t0 = srv_now();
  while (__atomic_load_n(&box->alive, __ATOMIC_ACQUIRE) == 0u) {
    /* a wave that has already served the pending request and left again also counts */
    if (__atomic_load_n(&box->ack_seq, __ATOMIC_ACQUIRE) == m->srv_seq && hipStreamQuery(m->srv_stream) == hipSuccess) break;
    if (srv_now() - t0 > 10.0) return set_err(CSGPU_E_HIP, "the single-node server did not start");
  }
  return CSGPU_OK;
}

/* wait for the server's stream by polling (hipStreamSynchronize on a kernel that has run for long sleeps in the kernel
 * driver and is woken milliseconds late: the solution check of a queens-64 search took 9 ms instead of 2) */
static void server_reap(csgpu_model *m) {
  const double t0 = srv_now();
  for (;;) {
    const hipError_t e = hipStreamQuery(m->srv_stream);
    if (e != hipErrorNotReady) break;
    if (srv_now() - t0 > 5.0) { (void)hipStreamSynchronize(m->srv_stream); break; }
  }
}

static void server_stop(csgpu_model *m) {
  if (m->h_box == NULL || !m->srv_launched) return;
  cs_mailbox_head *box = srv_box(m);
  __atomic_store_n(&box->stop, 1u, __ATOMIC_RELEASE);
  server_reap(m);
  __atomic_store_n(&box->stop, 0u, __ATOMIC_RELEASE);
  m->srv_launched = 0;
}

/* one node through the mailbox; trace == NULL: no trail wanted */
static int server_call(csgpu_model *m, const csgpu_val *state, csgpu_node node, csgpu_val *state_out, csgpu_result *result,
                       int32_t *trace, int32_t cap, int32_t *count) {
  cs_mailbox_head *box = srv_box(m);
  const size_t nbytes = (size_t)m->host->n_vars * sizeof(cs_val);
  const double t0 = srv_now();
  memcpy(m->h_box + m->box_state_off, state, nbytes);
  box->node.var = node.var; box->node.lo = node.lo; box->node.hi = node.hi; box->node.parent = 0;
  box->want_trace = trace != NULL ? 1u : 0u;
  const unsigned seq = ++m->srv_seq;
  const double t1 = srv_now();
  __atomic_store_n(&box->req_seq, seq, __ATOMIC_RELEASE);
  double t_start = 0.0;
  if (__atomic_load_n(&box->alive, __ATOMIC_ACQUIRE) == 0u) {
    const double ts = srv_now();
    const int rc = server_start(m);
    if (rc != CSGPU_OK) return rc;
    t_start = srv_now() - ts;
  }
  unsigned spins = 0;
  while (__atomic_load_n(&box->ack_seq, __ATOMIC_ACQUIRE) != seq) {
    if ((++spins & 0xfffu) == 0u) {
      /* the wave may have left (idle for too long) just before the request arrived: start another, which finds it */
      if (__atomic_load_n(&box->alive, __ATOMIC_ACQUIRE) == 0u && __atomic_load_n(&box->ack_seq, __ATOMIC_ACQUIRE) != seq) {
        const double ts = srv_now();
        const int rc = server_start(m);
        if (rc != CSGPU_OK) return rc;
        t_start += srv_now() - ts;
      }
      if (srv_now() - t1 > 30.0) return set_err(CSGPU_E_HIP, "the single-node server does not answer");
    }
  }
  const double t2 = srv_now();
  result->status = box->result.status; result->props = box->result.props;
  result->revisions = box->result.revisions; result->rounds = box->result.rounds;
  if (result->status >= 0) memcpy(state_out, m->h_box + m->box_out_off, nbytes);
  if (trace != NULL) {
    const unsigned made = box->trace_n;
    *count = (int32_t)made;
    unsigned kept = made < CS_SHAVE_TRACE_LDS ? made : CS_SHAVE_TRACE_LDS;
    if (kept > (unsigned)cap) kept = (unsigned)cap;
    memcpy(trace, m->h_box + m->box_trace_off, (size_t)kept * 16);
  }
  const double t3 = srv_now();
  m->srv_seconds[0] += t1 - t0;
  m->srv_seconds[1] += t2 - t1 - t_start;
  m->srv_seconds[2] += t3 - t2;
  m->srv_seconds[3] += t_start;
  m->srv_calls++;
  return CSGPU_OK;
}

extern "C" int csgpu_internal_server_warm(csgpu_model *m) {
  if (m == NULL || !m->finalized || !server_usable(m)) return CSGPU_OK;
  if (__atomic_load_n(&srv_box(m)->alive, __ATOMIC_ACQUIRE) != 0u) return CSGPU_OK;
  return server_start(m);
}

/* where the time of the single-node calls went: seconds[0..3] = host copy in, ring + wait, copy out, server (re)starts;
 * calls, starts.  For the launch path (CSGPU_SERVER=0): copy in, launch submit, wait, copy out (starts = 0). */
extern "C" int csgpu_debug_one_timing(const csgpu_model *m, double *seconds, uint64_t *calls, uint64_t *starts) {
  if (m == NULL || seconds == NULL || calls == NULL || starts == NULL) return set_err(CSGPU_E_ARG, "null argument");
  for (int i = 0; i < 4; i++) seconds[i] = m->srv_seconds[i];
  *calls = m->srv_calls;
  *starts = m->srv_starts;
  return CSGPU_OK;
}

extern "C" int csgpu_propagate_one_causes(const csgpu_model *cm, const csgpu_val *state, csgpu_node node,
                                          csgpu_val *state_out, csgpu_result *result, int32_t *trace, int32_t cap,
                                          int32_t *count) {
  csgpu_model *m = const_cast<csgpu_model *>(cm);
  if (m == NULL || state == NULL || state_out == NULL || result == NULL || trace == NULL || cap < 1 || count == NULL)
    return set_err(CSGPU_E_ARG, "bad argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (!kernel_qualifies(m, 7)) return set_err(CSGPU_E_LIMIT, "model does not qualify for the interval-only shaving kernel");
  if (server_usable(m)) return server_call(m, state, node, state_out, result, trace, cap, count);
  if (m->trace_cap < cap) {
    if (m->h_trace != NULL) (void)hipHostFree(m->h_trace);
    m->h_trace = NULL;
    HIP_TRY(hipHostMalloc((void **)&m->h_trace, (size_t)cap * 16 + 16, hipHostMallocMapped));
    m->h_trace_n = (unsigned *)(m->h_trace + (size_t)cap * 4);
    m->trace_cap = cap;
  }
  const size_t nbytes = (size_t)m->host->n_vars * sizeof(cs_val);
  const size_t part = (nbytes + 63) & ~(size_t)63;
  node.parent = 0;
  const double tl0 = srv_now();
  memcpy(m->h_one, state, nbytes);
  memcpy(m->h_one + part, &node, sizeof node);
  *m->h_trace_n = 0u;
  void *dev = NULL;
  HIP_TRY(hipHostGetDevicePointer(&dev, m->h_trace, 0));
  int4 *d_trace = (int4 *)dev;
  unsigned *d_trace_n = (unsigned *)((int32_t *)dev + (size_t)m->trace_cap * 4);
  unsigned ucap = (unsigned)cap;
  int n = m->host->n_vars, slots = m->img->dense_slots, dmin_d = m->img->dense_dmin, csz = 1;
  const void *tab_d = m->d_dense_tab;
  const int *root_lo_d = m->d_root_lo, *sym_off = m->d_sym_off;
  long long nb_d = 1;
  const uint64_t *d_batch = NULL;
  unsigned *tickets = NULL;
  const csgpu_val *d_in = (const csgpu_val *)m->d_one_in;
  const csgpu_node *d_node = (const csgpu_node *)m->d_one_node;
  csgpu_val *d_out = (csgpu_val *)m->d_one_out;
  csgpu_result *d_res = (csgpu_result *)m->d_one_res;
  void *args[] = { &n, &tab_d, &slots, &dmin_d, &root_lo_d, &sym_off, &d_in, &d_node, &d_out, &d_res,
                   &nb_d, &d_batch, &csz, &tickets, &d_trace, &d_trace_n, &ucap };
  const cs_planned *k = &m->plan.shave_trace;
  if (k->fn == NULL) return set_err(CSGPU_E_LIMIT, "no room in LDS for the trail next to the pair table");
  const double tl1 = srv_now();
  HIP_TRY(hipLaunchKernel(k->fn, dim3(1), dim3((unsigned)(k->waves * CS_WAVE)), args, k->lds, (hipStream_t)NULL));
  const double tl2 = srv_now();
  { const int rcw = wait_null_stream(); if (rcw != CSGPU_OK) return rcw; }
  const double tl3 = srv_now();
  memcpy(result, m->h_one + part + 64, sizeof *result);
  if (result->status >= 0) memcpy(state_out, m->h_one + part + 128, nbytes);
  const unsigned made = *m->h_trace_n;
  *count = (int32_t)made;
  unsigned kept = made < CS_SHAVE_TRACE_LDS ? made : CS_SHAVE_TRACE_LDS; /* what the kernel's LDS buffer holds */
  if (kept > (unsigned)cap) kept = (unsigned)cap;
  memcpy(trace, m->h_trace, (size_t)kept * 16);
  m->srv_seconds[0] += tl1 - tl0; m->srv_seconds[1] += tl2 - tl1; m->srv_seconds[2] += tl3 - tl2; m->srv_seconds[3] += srv_now() - tl3;
  m->srv_calls++;
  return CSGPU_OK;
}

/* ---- the reference's own failure chain of one node (cs_chain.hip.h) ---- */
#define CS_CHAIN_FRAMES (1 << 16)
#define CS_CHAIN_BUMPS 4096

/* operand of NOT(EQ(l, r)): a variable, or `variable + constant` with the constant on the right */
static int chain_operand(const cs_model *h, int32_t node, int *x, int *c) {
  const cs_node *nd = &h->nodes[node];
  if (nd->op == CS_OP_VAR) { *x = nd->a; *c = 0; return 1; }
  if (nd->op == CS_OP_ADD) {
    const cs_node *l = &h->nodes[nd->a], *r = &h->nodes[nd->b];
    if (l->op == CS_OP_VAR && r->op == CS_OP_CONST && r->a == r->b) { *x = l->a | CS_CHAIN_ADD; *c = r->a; return 1; }
  }
  return 0;
}

static int chain_build(csgpu_model *m) {
  if (m->chain_state != 0) return m->chain_state;
  const cs_model *h = m->host;
  m->chain_state = -1;
  if (!m->finalized || h->n_clauses < 1 || h->n_clauses > 60000 || h->n_vars < 1 || h->list_off == NULL) return -1;
  if ((size_t)h->n_vars * sizeof(cs_val) + (size_t)h->n_clauses * 2 + 64 > CS_CU_LDS) return -1;
  cs_chain_clause *cl = (cs_chain_clause *)malloc((size_t)h->n_clauses * sizeof *cl);
  if (cl == NULL) return -1;
  for (int32_t c = 0; c < h->n_clauses; c++) {
    const cs_node *top = &h->nodes[h->clause_node[c]];
    if (top->op == CS_OP_CONST) { /* a constant element of the root (a folded bound): in no variable's list */
      cl[c].lx = -1; cl[c].lc = 0; cl[c].rx = -1; cl[c].rc = 0;
      continue;
    }
    int ok = top->op == CS_OP_NOT && h->nodes[top->a].op == CS_OP_EQ;
    if (ok) {
      const cs_node *eq = &h->nodes[top->a];
      ok = chain_operand(h, eq->a, &cl[c].lx, &cl[c].lc) && chain_operand(h, eq->b, &cl[c].rx, &cl[c].rc);
    }
    if (!ok) { free(cl); return -1; } /* another clause shape: the walk of cs_chain.hip.h does not cover it */
  }
  int rc = upload(cl, (size_t)h->n_clauses * sizeof *cl, (int **)&m->d_chain_cl);
  free(cl);
  if (rc == CSGPU_OK) rc = upload(h->list_off, ((size_t)h->n_vars + 1) * sizeof(int32_t), &m->d_chain_off);
  if (rc == CSGPU_OK) rc = upload(h->list, (size_t)(h->list_off[h->n_vars] ? h->list_off[h->n_vars] : 1) * sizeof(int32_t), &m->d_chain_list);
  if (rc != CSGPU_OK) return -1;
  if (hipMalloc((void **)&m->d_chain_frames, (size_t)CS_CHAIN_FRAMES * sizeof(cs_chain_frame)) != hipSuccess ||
      hipHostMalloc((void **)&m->h_chain_out, (4 + CS_CHAIN_BUMPS) * sizeof(int), hipHostMallocMapped) != hipSuccess ||
      hipFuncSetAttribute((const void *)cs_ne_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CS_CU_LDS) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  m->chain_state = 1;
  return 1;
}

extern "C" int csgpu_propagate_one_chain(const csgpu_model *cm, const csgpu_val *state, csgpu_node node, int32_t *status,
                                         int32_t *props_out, int32_t *bumps, int32_t cap, int32_t *count) {
  csgpu_model *m = const_cast<csgpu_model *>(cm);
  if (m == NULL || state == NULL || status == NULL || props_out == NULL || bumps == NULL || count == NULL || cap < 0)
    return set_err(CSGPU_E_ARG, "bad argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if (node.var < 0 || node.var >= m->host->n_vars) return set_err(CSGPU_E_ARG, "no such variable");
  if (chain_build(m) != 1)
    return set_err(CSGPU_E_LIMIT, "the model is not a network of NOT(EQ(x [+ c], y [+ d])) clauses: no reference-order walk");
  const size_t nbytes = (size_t)m->host->n_vars * sizeof(cs_val);
  memcpy(m->h_one, state, nbytes); /* the mapped staging area of the single-node calls */
  void *dev = NULL;
  HIP_TRY(hipHostGetDevicePointer(&dev, m->h_chain_out, 0));
  int *d_out = (int *)dev, *d_bumps = (int *)dev + 4;
  cs_node_in nd;
  nd.var = node.var; nd.lo = node.lo; nd.hi = node.hi; nd.parent = 0;
  const size_t lds = ((nbytes + 15) & ~(size_t)15) + (((size_t)m->host->n_clauses * 2 + 15) & ~(size_t)15);
  hipLaunchKernelGGL(cs_ne_chain, dim3(1), dim3(64), lds, (hipStream_t)NULL, m->host->n_vars, m->host->n_clauses,
                     (const cs_chain_clause *)m->d_chain_cl, (const int *)m->d_chain_off, (const int *)m->d_chain_list,
                     (const cs_val *)m->d_one_in, nd, m->d_chain_frames, (int)CS_CHAIN_FRAMES, d_out, d_bumps, (int)CS_CHAIN_BUMPS);
  HIP_TRY(hipGetLastError());
  { const int rcw = wait_null_stream(); if (rcw != CSGPU_OK) return rcw; }
  if (m->h_chain_out[3] != 0) return set_err(CSGPU_E_LIMIT, "the reference-order walk overflowed its frame stack or its bump list");
  *status = m->h_chain_out[0];
  *props_out = m->h_chain_out[1];
  const int made = m->h_chain_out[2];
  *count = made;
  memcpy(bumps, m->h_chain_out + 4, (size_t)(made < cap ? made : cap) * sizeof(int32_t));
  return CSGPU_OK;
}

extern "C" int csgpu_propagate_one(const csgpu_model *m, const csgpu_val *state, csgpu_node node, csgpu_val *state_out,
                                   csgpu_result *result) {
  if (m == NULL || state == NULL || state_out == NULL || result == NULL) return set_err(CSGPU_E_ARG, "null argument");
  if (!m->finalized) return set_err(CSGPU_E_STATE, "model is not finalized");
  if ((m->kernel_choice == 0 || m->kernel_choice == 7) && kernel_qualifies(m, 7) && server_usable(const_cast<csgpu_model *>(m)))
    return server_call(const_cast<csgpu_model *>(m), state, node, state_out, result, NULL, 0, NULL);
  const size_t nbytes = (size_t)m->host->n_vars * sizeof(cs_val);
  const size_t part = (nbytes + 63) & ~(size_t)63;
  node.parent = 0;
  memcpy(m->h_one, state, nbytes);
  memcpy(m->h_one + part, &node, sizeof node);
  int rc = csgpu_propagate_batch(m, (const csgpu_val *)m->d_one_in, (const csgpu_node *)m->d_one_node,
                                 (csgpu_val *)m->d_one_out, (csgpu_result *)m->d_one_res, 1, NULL);
  if (rc != CSGPU_OK) return rc;
  { const int rcw = wait_null_stream(); if (rcw != CSGPU_OK) return rcw; } /* one launch, one wait: the kernel worked on the mapped host buffers */
  memcpy(result, m->h_one + part + 64, sizeof *result);
  if (result->status >= 0) memcpy(state_out, m->h_one + part + 128, nbytes);
  return CSGPU_OK;
}
