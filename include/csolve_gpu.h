/* csolve_gpu.h -- C ABI of libcsolve_hip.so: the MI355X (gfx950) implementation of
 * CSolve's constraint-propagation fixpoint.
 *
 * Plain C, plain pointers and sizes.  Device pointers are raw HIP device addresses
 * (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void* (NULL =
 * the null stream).  Every entry returns 0 on success or a negative CSGPU_E_* code;
 * csgpu_last_error() gives the message.  There is no CPU fallback anywhere behind
 * this interface: without a usable HIP device the calls fail with CSGPU_E_HIP.
 *
 * What each entry replaces in the reference (jeuneS2/csolve, paths under src/):
 *
 *   csgpu_model_from_text / _from_file    the text front end up to the point where the
 *                                         trees exist: lexer.l:36-102, parser.y:94-283
 *   csgpu_model_root_propagate            propagate(root, size) of the Input action,
 *                                         parser.y:59,67 -> propagate.c:474-485 (sweeps of
 *                                         propagate_wand 379-392 over all top-level clauses)
 *   csgpu_model_finalize                  env_generate + clauses_init, parser.y:81-83 ->
 *                                         parser_support.c:245-257, 338-396
 *   csgpu_propagate_batch                 check_assignment -> propagate_clauses(&var->clauses),
 *                                         csolve.c:247-261 -> propagate.c:488-538, for a whole
 *                                         batch of search nodes at once; each node is
 *                                         step_enter's bind(var, VALUE(v)) (csolve.c:294-304)
 *                                         followed by the event-driven fixpoint
 *   csgpu_eval_batch                      update_solution's eval of the root, csolve.c:226 ->
 *                                         eval.c:233-255 (and everything below it, eval.c:27-230)
 *
 * The csolve.h-named drop-in symbols (propagate, propagate_clauses, eval_*, ...) live in
 * libcsolve_dropin.so, declared in include/csolve_dropin.h, and are thin shims over this ABI.
 */
#ifndef CSOLVE_GPU_H
#define CSOLVE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSGPU_OK 0
#define CSGPU_E_ARG (-1)      /* bad argument */
#define CSGPU_E_PARSE (-2)    /* problem text rejected (message has the reference's wording) */
#define CSGPU_E_HIP (-3)      /* HIP runtime error / no device */
#define CSGPU_E_LIMIT (-4)    /* model exceeds a device-side limit */
#define CSGPU_E_STATE (-5)    /* call out of order (e.g. propagate before finalize) */
#define CSGPU_E_UNBOUNDED (-6) /* env_generate: "unbounded variable: %s" */

/* closed interval, layout of reference `struct val_t` (csolve.h:43-46) */
typedef struct csgpu_val {
  int32_t lo, hi;
} csgpu_val;

/* one search node of a batch: take state `parent` (or the identity index), set
 * variable `var` to [lo,hi] (a single value for step_enter, an interval for the
 * worker split of csolve.c:121-150), propagate.  var < 0: no assignment, every
 * variable counts as changed (full fixpoint). */
typedef struct csgpu_node {
  int32_t var, lo, hi, parent;
} csgpu_node;

/* per-node result.  status: -1 = PROP_ERROR (csolve.h:84); otherwise the node is consistent and
 * status = number of variables that are still open (not a single value), 0 = complete assignment.
 * props = narrowing events (the reference's PROPS counter, propagate.c:77-78),
 * revisions = clause revisions performed, rounds = worklist rounds -- and for an INCONSISTENT node (status -1)
 * the index of a variable whose domain became empty, or -1 if the kernel does not attribute the failure (kernels
 * 1, 6, 7 do; the reference bumps that variable's priority, propagate_term_confl, propagate.c:33-41; which of
 * several emptied variables is reported depends on the revision order; where an expression tree fails at a constant
 * and no domain is empty, kernels 1 and 6 report the first variable of that tree). */
typedef struct csgpu_result {
  int32_t status, props, revisions, rounds;
} csgpu_result;

typedef struct csgpu_model csgpu_model;

const char *csgpu_last_error(void);
/* number of visible HIP devices (0 or negative error); selects `device` for this thread */
int csgpu_device_count(void);
int csgpu_set_device(int device);

/* ---- host model ---- */
int csgpu_model_from_text(const char *text, int weights_on, csgpu_model **out);
int csgpu_model_from_file(const char *path, int weights_on, csgpu_model **out);
/* a golden-model file (csolve_amd/csrc/cs_model.c) with domains and clause lists already final */
int csgpu_model_from_dump(const char *path, csgpu_model **out);
void csgpu_model_free(csgpu_model *m);

int csgpu_model_num_vars(const csgpu_model *m);
int csgpu_model_num_clauses(const csgpu_model *m);
int csgpu_model_objective(const csgpu_model *m);        /* 0 ANY 1 ALL 2 MIN 3 MAX */
int csgpu_model_objective_var(const csgpu_model *m);    /* -1 if none */
const char *csgpu_model_var_name(const csgpu_model *m, int var);
/* copy the current root domains (host memory, n_vars entries) */
int csgpu_model_get_domains(const csgpu_model *m, csgpu_val *out);
int csgpu_model_set_domains(csgpu_model *m, const csgpu_val *in);
/* table sizes of the uploaded device image: [0] adjacency entries, [1] binary-NE clauses,
 * [2] tree clauses, [3] tree nodes, [4] LDS bytes per node instance, [5] max list length */
int csgpu_model_device_info(const csgpu_model *m, int64_t info[8]);

/* Root phase on the device: full sweeps over every top-level clause until nothing
 * changes.  *status = -1 if the problem is infeasible, else the number of narrowings.
 * The model's root domains are updated in place.  (The reference stops after limit+1
 * Gauss-Seidel sweeps, propagate.c:483; the device runs Jacobi rounds to the fixpoint,
 * which is the same state whenever the reference reaches its fixpoint within the limit.) */
int csgpu_model_root_propagate(csgpu_model *m, int32_t *status);
/* The same with the reference's `limit` (propagate.c:479-483: at most limit + 1 sweeps; limit < 0: none).  The
 * device's sweeps revise all clauses of a round in parallel, the reference's one after the other (Gauss-Seidel),
 * so k device rounds never narrow more than k reference sweeps: whenever the device reaches its fixpoint within
 * limit + 1 rounds (*rounds, if wanted, says how many it took) the reference does too and the states are equal;
 * when the limit cuts the device short the result is a sound but possibly wider state than the reference's. */
int csgpu_model_root_propagate_limit(csgpu_model *m, int64_t limit, int32_t *status, int32_t *rounds);

/* The root normalisation pass between the two root propagations (normalize(), reference
 * src/normalize.c:305-316, parser.y:66): a host-side rewrite of the trees (constant folding,
 * neutral elements, constants moved across `<`, double negation, De Morgan); no domain changes. */
int csgpu_model_normalize(csgpu_model *m);
/* SURVEY 8f-1 (the normaliser as a pre-pass that specialises the tables per subtree prefix): a new, unfinalized model
 * for the subtree below `state` (one interval per variable, inside the model's root domains; normally a consistent
 * state a search has reached): the same trees with `state` as root domains.  csgpu_model_normalize on it folds what the
 * prefix has decided (normalize.c:67-316), csgpu_model_root_propagate re-establishes the fixpoint, csgpu_model_finalize
 * leaves entailed clauses out of the device tables: shorter clause lists, the same results for every state inside
 * `state` (normalisation never changes results, only cost).  The new model is independent of `m`. */
int csgpu_model_specialize(const csgpu_model *m, const csgpu_val *state, csgpu_model **out);
/* A learnt conflict clause (struct confl_t, csolve.h:98-128; conflict_create, conflict.c:319-361): "not all of
 * vars[i] == values[i]".  It is evaluated like eval_confl (eval.c:258-277) and propagated like propagate_confl
 * (propagate.c:395-471: when every element but one has its conflict value, that value is shaved off the bound of
 * the remaining variable it sits on).  The clause becomes the last top-level clause and the last entry of its
 * variables' clause lists.  May be called before or after csgpu_model_finalize; afterwards the device tables are
 * rebuilt (the call costs O(model)) -- which frees the old ones: while a csgpu_search built on the model exists (its
 * kernels' arguments and captured graphs point into them) the call is refused with CSGPU_E_STATE; free the engines
 * first.  At most 255 elements (CSGPU_E_LIMIT). */
int csgpu_model_add_conflict(csgpu_model *m, int32_t count, const int32_t *vars, const int32_t *values);

/* eval_<op> on the current root domains, host buffers, no finalize needed (variables may
 * still be unbounded): vals[c] = interval value of clause c (eval.c:27-255).  Synchronous. */
int csgpu_model_eval_clauses_host(csgpu_model *m, csgpu_val *vals);

/* Host-only half of finalize: env_generate + clauses_init + construction of the device
 * tables in host memory (no HIP call).  csgpu_model_device_info works afterwards. */
int csgpu_model_build_tables(csgpu_model *m);

/* env_generate + clauses_init + upload of the search tables.  Fails with
 * CSGPU_E_UNBOUNDED if a variable still has an infinite bound. */
int csgpu_model_finalize(csgpu_model *m);

/* ---- sets-only states: the domains as bit vectors -------------------------------------------------------
 * For models that qualify for kernel 4 a search state can be carried as its forbidden sets alone
 * ([rows][n_vars][FW] 64-bit words, FW = csgpu_model_forbidden_words): every value outside a variable's
 * interval is marked in the variable's own set, so the interval is [lowest unmarked, highest unmarked] and
 * need not be stored.  Half the bytes per node of the interval + sets layout; same fixpoints, verdicts and
 * PROPS (tests unpack and compare).
 *   pack:    interval states -> sets (forbidden values of valued neighbours + everything outside the interval)
 *   unpack:  sets -> interval states ({1,0} for a variable with no allowed value)
 *   propagate_batch_sets: as csgpu_propagate_batch_fb, nodes[i].parent indexes d_sets_in; rows of inconsistent
 *   nodes in d_sets_out are unspecified.  CSGPU_E_LIMIT if the model does not qualify. */
int csgpu_sets_pack(const csgpu_model *m, const csgpu_val *d_states, uint64_t *d_sets, int64_t count, void *stream);
int csgpu_sets_unpack(const csgpu_model *m, const uint64_t *d_sets, csgpu_val *d_states, int64_t count, void *stream);
int csgpu_propagate_batch_sets(const csgpu_model *m, const uint64_t *d_sets_in, const csgpu_node *d_nodes,
                               uint64_t *d_sets_out, csgpu_result *d_results, int64_t batch, void *stream);

/* Kernel selection for the batched fixpoint: 0 = automatic (default), 1 = the general kernel
 * (adjacency read through L2; handles tree clauses), 2 = the LDS-resident unit-shaving kernel
 * (pure binary-NE models whose packed adjacency fits in LDS), 3 = the forbidden-set kernel (same
 * models, root intervals of at most 256 values), 4 = its register-resident variant (additionally
 * at most 256 variables and a dense pair table that fits in LDS), 5 = kernel 4 with two or four
 * nodes per wavefront (additionally at most 32 variables of at most 64 values; 4 then means one
 * node per wavefront), 6 = the clause-resident kernel for small models (at most 512 clauses: every
 * lane keeps its clauses in registers and a round revises all of them), 7 = the interval-only shaving
 * kernel (models that qualify for 4: bounds are shaved by pushes and moved bounds verified against the
 * valued variables through the symmetric pair table; no forbidden sets anywhere);
 * CSGPU_E_LIMIT if the model does not qualify.  All compute the same results; tests run every parity
 * case through each of them.
 * Automatic: csgpu_propagate_batch_fb (sets passed) uses 5 when the model qualifies, else 4, else 3;
 * csgpu_propagate_batch (states only) uses 5 with the sets rebuilt for models of at most 32 variables,
 * else 7, else 2 (more than 256 variables: rebuilding forbidden sets costs a list scan per valued variable of
 * every incoming state, the event-driven kernels scan one list per narrowing), else 6 (at most 256 clauses;
 * with 257-512 for batches of at most 8192 nodes only, where its lower latency counts and its lower throughput
 * does not), else 1. */
int csgpu_model_set_kernel(csgpu_model *m, int which);
/* Process-wide switch for models finalized afterwards: 1 (default) = EQ / LT / two-literal OR clauses
 * over `VAR` or `VAR + constant` operands are revised by direct bound propagation (schedule.txt-style
 * models then need no expression-tree interpreter); 0 = they stay expression trees.  Same fixpoints
 * either way (tests compare the two). */
void csgpu_set_linear_fast_paths(int on);
/* 1 if the finalized model can run kernel `which` (1..6), else 0 */
int csgpu_model_qualifies(const csgpu_model *m, int which);
/* which kernel csgpu_propagate_batch will launch (see above) */
int csgpu_model_get_kernel(const csgpu_model *m);

/* ---- batched propagation (the hot path) ----
 * d_states_in : device, [*][n_vars] csgpu_val   parent states
 * d_nodes     : device, [batch] csgpu_node      (parent = row of d_states_in)
 * d_states_out: device, [batch][n_vars] csgpu_val, row i = fixpoint of node i
 *               (left unwritten when the node fails)
 * d_results   : device, [batch] csgpu_result
 * Asynchronous on `stream`; no host synchronisation inside. */
int csgpu_propagate_batch(const csgpu_model *m, const csgpu_val *d_states_in, const csgpu_node *d_nodes,
                          csgpu_val *d_states_out, csgpu_result *d_results, int64_t batch, void *stream);

/* Same, with the incumbent bound of an optimisation run: before a node is propagated the
 * objective variable "<obj>" is intersected with [obj_lo, obj_hi] (objective_update_val,
 * objective.c:101-126) and, if that moved a bound, its clauses are propagated as well
 * (check_assignment, csolve.c:251-252).  Pass INT32_MIN / INT32_MAX for "no bound". */
int csgpu_propagate_batch_obj(const csgpu_model *m, const csgpu_val *d_states_in, const csgpu_node *d_nodes,
                              csgpu_val *d_states_out, csgpu_result *d_results, int64_t batch, int32_t obj_lo,
                              int32_t obj_hi, void *stream);

/* Forbidden-set variant (pure binary-NE models with root intervals of at most 256 values).
 * Besides its interval every variable carries FW = csgpu_model_forbidden_words(m) 64-bit words:
 * bit k set <=> value root_lo+k is forbidden by a neighbour that is a single value.  The sets are
 * derived data that the search keeps next to each state so that a child inherits them:
 *   d_forb_in  [*][n_vars][FW] uint64, rows parallel to d_states_in  (NULL: rebuild from the state)
 *   d_forb_out [batch][n_vars][FW] uint64, rows parallel to d_states_out (NULL: not wanted)
 * Results (fixpoints, verdicts, PROPS of consistent nodes) are those of csgpu_propagate_batch.
 * Rows of inconsistent nodes (status -1) in d_states_out / d_forb_out are unspecified: the register-resident
 * kernel stores them unconditionally, the other kernels leave them untouched.  Bits of values outside a
 * variable's root domain are unspecified as well (a push may or may not be recorded there); they never
 * influence a result, and sets written by one kernel may be fed to another. */
int csgpu_model_forbidden_words(const csgpu_model *m); /* 0: the model does not qualify */
int csgpu_propagate_batch_fb(const csgpu_model *m, const csgpu_val *d_states_in, const uint64_t *d_forb_in,
                             const csgpu_node *d_nodes, csgpu_val *d_states_out, uint64_t *d_forb_out,
                             csgpu_result *d_results, int64_t batch, void *stream);

/* ---- many instances of one model in one call: a depth-first search per wavefront ----
 * For models that qualify for kernel 7 (csgpu_model_qualifies(m, 7): a pure != network of at most 256 variables whose
 * dense pair table fits LDS).  An instance is a row of root domains d_roots[i][n_vars] INSIDE the model's own root
 * domains (same clauses, other givens -- e.g. the empty sudoku model and one row of givens per puzzle).  One wavefront
 * takes an instance from its root row to its answer: the root node (every valued variable pushes), then depth-first
 * with the engine's default rule (the open variable with the smallest interval, ties to the lowest index; values in
 * ascending order; a child is the assignment followed by the fixpoint).  Instances are drawn by ticket; the launch
 * keeps no more than the resident waves of the device busy, whatever `count` is.
 *   options->objective  0 ANY: stop at an instance's first solution; 1 ALL: walk its whole tree and count
 *   options->max_nodes  budget per instance (children tried), > 0: there is no "unlimited".  An instance that would
 *                       need one more node stops with status CSGPU_MANY_LIMIT, nodes == max_nodes and the counters
 *                       of what it did; the caller re-runs such an instance through a csgpu_search, or uses
 *                       csgpu_solve_many_checkpointed (below), which lets it go on from where it stopped
 *   d_results[i]        status; nodes = children tried (a value that a valued neighbour forbids is a node and a cut),
 *                       cuts = inconsistent children, props = narrowings of the consistent children (the reference's
 *                       PROPS on such networks), solutions; root_props = narrowings of the root node (0 when the root
 *                       is inconsistent).  An inconsistent root is no error: CSGPU_MANY_DONE, 0 nodes, 0 solutions.
 *                       A row outside the model's root domains, or with lo > hi, is CSGPU_MANY_BAD_ROOT and is not
 *                       searched (the device tables are relative to the root domains, and finalize has dropped the
 *                       clauses that are true on all of them)
 *   d_solutions         NULL, or [count][n_vars] int32: row i receives the FIRST solution of instance i (ANY and ALL);
 *                       rows of instances without a solution are left untouched
 * Device pointers; asynchronous on `stream`, no host synchronisation inside once the model's workspace exists.  That
 * workspace (the waves' stacks: waves x n_vars frames x (n_vars + 1) x 8 bytes with min(count, resident waves) waves,
 * and the ticket counters, which the kernel leaves at zero) belongs to the model: it is allocated by the first call,
 * grown by a call that launches more waves, and freed with the model.  Hence ONE call in flight per model: a second
 * call may be queued behind the first on the same stream, never on another stream or from another thread.
 * Errors before any HIP call: null model / roots / results / options, count < 0, max_nodes <= 0 -> CSGPU_E_ARG;
 * objective MIN / MAX -> CSGPU_E_LIMIT; model not finalized -> CSGPU_E_STATE; model does not qualify for kernel 7 ->
 * CSGPU_E_LIMIT.  count == 0 -> CSGPU_OK, nothing is launched. */
#define CSGPU_MANY_DONE 0     /* ANY: solved, or proven to have no solution; ALL: whole tree walked */
#define CSGPU_MANY_LIMIT 1    /* stopped at max_nodes; the counters hold what was done */
#define CSGPU_MANY_BAD_ROOT 2 /* row outside the model's root domains, or lo > hi: not searched */
typedef struct csgpu_many_result {
  int32_t status, root_props;
  int64_t nodes, cuts, props, solutions;
} csgpu_many_result;
typedef struct csgpu_many_options {
  int32_t objective; /* 0 ANY, 1 ALL */
  int32_t reserved;  /* 0 */
  int64_t max_nodes;
} csgpu_many_options;
int csgpu_solve_many(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_options *options,
                     csgpu_many_result *d_results, int32_t *d_solutions, void *stream);

/* ---- checkpoints: csgpu_solve_many in slices ----
 * An instance that stops at max_nodes with work left keeps what it walked: it draws a slot of a pool and leaves there its
 * frame stack, its current node and {branching variable, next value}.  From the slot it goes on in two ways:
 *   csgpu_solve_many_resume        on a wavefront again, with a budget for THIS call (nodes tried in the call); the
 *                                  counters accumulate and the first solution is stored when `solutions` goes from 0 to
 *                                  1, so a walk in slices gives, field for field, the one call with the summed budget
 *   csgpu_many_checkpoint_states   its open subtrees as states, for a csgpu_search that puts the whole device on them
 * csgpu_solve_many_checkpointed is csgpu_solve_many plus the pool: d_slots[i] receives the slot of an instance that stopped
 * with a checkpoint, and -1 for every other one (DONE, BAD_ROOT, or LIMIT while the pool had no slot left -- such an
 * instance ends exactly as in csgpu_solve_many).  csgpu_solve_many_resume takes the same d_results / d_solutions /
 * d_slots rows: an instance with d_slots[i] < 0 is left untouched (nothing of it is written); one with a slot reads its
 * counters from d_results[i], goes on, and ends DONE (d_slots[i] = -1) or LIMIT (the checkpoint goes back into the SAME
 * slot).  A slot number outside [0, capacity), or a slot that holds no checkpoint, gives status CSGPU_MANY_BAD_SLOT and
 * nothing else of the instance is touched (the kernel compares before it reads).
 * Slots are not recycled one by one: a slot stays with its instance until csgpu_many_checkpoints_reset makes every slot
 * free again.  A caller that runs K instances in slices creates the pool with as many slots as it will let stop, K at
 * the most.  A slot is csgpu_many_checkpoint_bytes(m) bytes: (n_vars + 1) frames of (n_vars + 1) 8-byte entries.
 * Concurrency: "one call in flight per model" holds for these calls too (they share the model's ticket counters); the
 * same slot number twice in one resume call is undefined; the pool must outlive the calls queued on it and is freed
 * before its model.
 * Errors before any HIP call, as csgpu_solve_many: a null pointer (d_solutions may be null), count < 0, max_nodes <= 0,
 * capacity < 1 -> CSGPU_E_ARG; MIN / MAX -> CSGPU_E_LIMIT; model not finalized -> CSGPU_E_STATE; model does not qualify
 * -> CSGPU_E_LIMIT; a pool created for another model -> CSGPU_E_ARG.
 * csgpu_many_checkpoint_states: the open subtrees of one checkpoint, the oldest frame (the largest subtree) first: a
 * frame {row, bv, next} becomes row with bv narrowed to [next, row[bv].hi], the current node the same with its next
 * value.  *count = depth + 1; CSGPU_E_LIMIT (and *count set) if cap is smaller; CSGPU_E_STATE if the slot holds no
 * checkpoint.  It reads the slot's header on `stream` and waits for it.  The states are NOT at the fixpoint yet: `next`
 * has not been pushed, and when it is the variable's last value the state has a new valued variable.  Run them through
 * csgpu_propagate_batch as `var < 0` nodes and drop the inconsistent ones before csgpu_search_put; a state that is fully
 * valued after that is a solution of its own and must not be put (the engine branches on an open variable): count it. */
#define CSGPU_MANY_BAD_SLOT 3 /* csgpu_solve_many_resume: d_slots[i] names no checkpoint of the pool: not touched */
typedef struct csgpu_many_checkpoints csgpu_many_checkpoints; /* device pool, belongs to one finalized model */
size_t csgpu_many_checkpoint_bytes(const csgpu_model *m); /* bytes per slot; 0 if the model does not qualify.  No HIP call:
                                                             after finalize, or after csgpu_model_build_tables alone */
int csgpu_many_checkpoints_create(const csgpu_model *m, int64_t capacity, csgpu_many_checkpoints **out);
int csgpu_many_checkpoints_reset(csgpu_many_checkpoints *ck, void *stream); /* every slot free again */
void csgpu_many_checkpoints_free(csgpu_many_checkpoints *ck);
int csgpu_solve_many_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_options *options,
                                  csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck,
                                  int32_t *d_slots, void *stream);
int csgpu_solve_many_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options, csgpu_many_result *d_results,
                            int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_many_checkpoint_states(const csgpu_many_checkpoints *ck, int32_t slot, csgpu_val *d_states, int64_t cap, int64_t *count,
                                 void *stream);

/* ---- stopped ALL walks spread over the waves of the next call ----
 * A launch lasts as long as its deepest instance while the other waves idle.  A checkpoint holds what splits such a
 * walk: every frame is "node, branching variable bv, next value", and the walk's untried children are, in WALK ORDER,
 * the values next .. hi(bv) of the current node (ascending), then those of the frame below it, down to the oldest frame.
 * Each child -- the frame's node in absolute bounds with bv = [v, v] -- is a root row that csgpu_solve_many[_checkpointed]
 * walks like any other, and its record gives its owner, exactly (ALL only):
 *   nodes += 1 + sub.nodes;  cuts += sub.cuts + (the row was inconsistent as a root: DONE, 0 nodes, 0 solutions);
 *   props += sub.root_props + sub.props;  solutions += sub.solutions
 * (the fixpoint of a != network is unique, props counts units shaved, and the assignment itself is counted on neither
 * side).  Summed over all children, over any number of levels, that is the record of the one ALL call, field for field;
 * the first solution in row order is the walk's first.
 *   csgpu_many_checkpoint_children   d_children[i] = the children of the checkpoint in slot d_slots[i] (int64 [count]):
 *                                    0 for d_slots[i] < 0; -1 for a slot that is refused: a number >= capacity, a header
 *                                    without a checkpoint or with a depth outside [0, n_vars), a frame whose variable is
 *                                    outside [0, n_vars), whose node's bounds of it lie outside the root domain or whose
 *                                    next value lies outside those bounds.  Everything is compared before what depends
 *                                    on it is read; a refused slot is never a count
 *   csgpu_many_checkpoint_fanout     d_offsets: int64 [count + 1], the exclusive prefix sum of the counts (refused ones as
 *                                    0), on the device: no host round trip in between.  Instance i writes its children
 *                                    to rows d_offsets[i] .. of d_rows ([total][n_vars]) in walk order and, if d_owner is
 *                                    not NULL, d_owner[row] = i (int32 [total]).  It counts its slot again first and
 *                                    writes NOTHING unless d_offsets[i + 1] - d_offsets[i] is that count and the rows lie
 *                                    inside [0, total).  The rows are copies: the pool may be reset once this has run
 *   csgpu_many_fold                  d_results[d_owner[t]] += the contribution above of d_sub_results[t], t < total, with
 *                                    relaxed device-scope 64-bit adds; status and root_props of the owner are not touched,
 *                                    d_owner[t] < 0 is skipped.  Folding a record twice counts it twice: a batch is
 *                                    folded exactly once, when the caller leaves it.  Owners across levels: map a row's
 *                                    owner through the owner vector of the level before.  It takes no pool and knows no
 *                                    model: the clause family's spread (csgpu_many_clause_checkpoint_children /
 *                                    _fanout below) folds with this same call
 * All three are asynchronous on `stream` and read the pool only; they take a pool of csgpu_many_checkpoints_create.
 * Errors before any HIP call, in this order: a null pointer (d_owner of the fan-out may be null) -> CSGPU_E_ARG; count < 0
 * or total < 0 -> CSGPU_E_ARG; a pool of csgpu_many_clause_checkpoints_create -> CSGPU_E_ARG; count > 2^31 - 1 ->
 * CSGPU_E_LIMIT.  Then count == 0 or total == 0 -> CSGPU_OK, nothing is launched. */
int csgpu_many_checkpoint_children(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count, int64_t *d_children,
                                   void *stream);
int csgpu_many_checkpoint_fanout(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count, const int64_t *d_offsets,
                                 csgpu_val *d_rows, int32_t *d_owner, int64_t total, void *stream);
int csgpu_many_fold(const csgpu_many_result *d_sub_results, const int32_t *d_owner, int64_t total, csgpu_many_result *d_results,
                    void *stream);

/* ---- up to k solutions per instance: csgpu_solve_many, left at an instance's k-th solution ----
 * "Is the solution unique?", "give me the first k": the instance walks exactly the ALL walk (same branching rule, same
 * value order, same counters) and stops right after accepting its k-th solution, as ANY stops after its first.
 * max_solutions = 1 is ANY, field for field; an instance whose whole tree holds fewer than k solutions ends as under
 * ALL, field for field.  d_results is csgpu_many_result as above.  CSGPU_MANY_DONE: the k-th solution was reached or the
 * tree is exhausted, and solutions == min(k, solutions of the tree) -- with k = 2, "unique" is DONE && solutions == 1,
 * "several" DONE && solutions == 2, "none" DONE && solutions == 0.  LIMIT, BAD_ROOT and BAD_SLOT are as above.
 *   d_solutions   NULL, or [count][max_solutions][n_vars] int32: row j of instance i is its j-th solution in walk order
 *                 (a root row that is a solution already is row 0); rows >= solutions of an instance are not touched
 * The three entries are csgpu_solve_many, csgpu_solve_many_checkpointed and csgpu_solve_many_resume with this stop; pool,
 * slots, csgpu_many_checkpoint_states and csgpu_many_checkpoints_reset are those above, unchanged, and a checkpoint
 * written here exports its open subtrees like any other.  A resumed instance reads its counters from its record and
 * continues its rows at index `solutions`: a walk in slices gives, field for field and row for row, the one call with
 * the summed budget.  max_solutions is per call: a resumed instance whose record already has solutions >= max_solutions
 * ends DONE before it tries a node, and nothing of it is written but its status and d_slots[i] = -1 (rows are indexed
 * with the max_solutions of the call that writes them: give every slice the k the buffer was laid out for, or a buffer
 * laid out for the new k).  "One call in flight per model" covers these calls (same workspace, same ticket counters);
 * calls of both families may be queued behind each other on one stream without the host in between.
 * Errors before any HIP call, in csgpu_solve_many's order: a null pointer (d_solutions may be null), count < 0,
 * max_nodes <= 0, max_solutions < 1 -> CSGPU_E_ARG; model not finalized -> CSGPU_E_STATE; model does not qualify for
 * kernel 7 -> CSGPU_E_LIMIT; a pool created for another model -> CSGPU_E_ARG.  count == 0 -> CSGPU_OK, nothing is
 * launched. */
typedef struct csgpu_many_upto_options {
  int32_t max_solutions; /* k >= 1: an instance stops at its k-th solution */
  int32_t reserved;      /* 0 */
  int64_t max_nodes;     /* as csgpu_many_options */
} csgpu_many_upto_options;
int csgpu_solve_many_upto(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_upto_options *options,
                          csgpu_many_result *d_results, int32_t *d_solutions, void *stream);
int csgpu_solve_many_upto_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                       const csgpu_many_upto_options *options, csgpu_many_result *d_results, int32_t *d_solutions,
                                       csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_solve_many_upto_resume(const csgpu_model *m, int64_t count, const csgpu_many_upto_options *options,
                                 csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots,
                                 void *stream);

/* ---- branching on the allowed values: csgpu_solve_many that skips what a valued neighbour forbids ----
 * csgpu_solve_many branches on the smallest INTERVAL and tries every value of it; a value that a valued neighbour forbids
 * is a node and a cut.  That makes its counters the engine's, but on a != network an interval hides holes: a variable
 * with bounds [1, 9] of which only 1 and 9 are still possible looks like the widest of the board.  These two calls walk
 * with the classic forward-checking rule instead.  Opt-in: another tree, the same set of solutions.
 * The walk is exactly csgpu_solve_many's except for the branching.  Unchanged: the root check and BAD_ROOT; the root node
 * (every valued variable pushes) and root_props; a child is the assignment followed by the same interval fixpoint;
 * max_nodes is compared before a child is tried; ANY / ALL / DONE / LIMIT; the first solution is stored.  At a node (a
 * fixpoint with open variables), for an open variable w with bounds [lo, hi]:
 *   forbidden value   c in [lo, hi] is forbidden if some VALUED variable u and some clause w + a != u + b of the model, in
 *                     any slot of the pair, has c + a == value(u) + b
 *   allowed(w)        the other values of [lo, hi].  At a fixpoint lo and hi are always allowed (the fixpoint has found
 *                     them supported), so |allowed(w)| >= 2, its first value is lo and its last is hi
 *   branching         the open variable with the smallest |allowed(w)|, ties to the lowest index; its allowed values in
 *                     ascending order.  A forbidden value is NOT a node: it is neither tried nor counted
 *   counters          keep their definitions: nodes = children tried, cuts = inconsistent children, props = narrowings of
 *                     the consistent children, solutions
 *   frames            a frame is pushed when the node has an allowed value left after the one being entered; none for
 *                     the last value, which is hi.  A frame stays {row, variable, next = value + 1}: coming back to it
 *                     the walk recomputes allowed(variable) on the frame's row and goes on at the first allowed value
 *                     >= next.  The workspace is csgpu_solve_many's, formula and all
 * Domains stay intervals and the fixpoint is untouched: no interior value is ever removed from a domain.
 * csgpu_solve_many_allowed is csgpu_solve_many with this walk; csgpu_solve_many_allowed_upto is csgpu_solve_many_upto
 * with it (rows [count][max_solutions][n_vars] in walk order, rows >= solutions untouched, max_solutions = 1 is the ANY
 * call field for field, an instance with fewer than k solutions ends as under ALL).  Which models qualify
 * (csgpu_model_qualifies_many_allowed, usable after csgpu_model_build_tables alone): kernel 7's rule, and no root domain
 * of more than 128 values, which is what the kernels' allowed sets hold.
 * Not on this walk (use the width rule): restarts, the solution stream, and the clause family; the csgpu_search
 * strategies are not touched either.  Checkpoints, resume and the spread of stopped instances: the calls further down.
 * "One call in flight per model" covers these calls (same workspace, same ticket counters, left at zero); calls of the
 * whole family may be queued behind each other on one stream.
 * Errors before any HIP call are those of csgpu_solve_many (csgpu_solve_many_upto for the second call), in their order;
 * in addition a finalized model that qualifies for kernel 7 but has a root domain of more than 128 values ->
 * CSGPU_E_LIMIT with a message that says so.  count == 0 -> CSGPU_OK, nothing is launched. */
int csgpu_model_qualifies_many_allowed(const csgpu_model *m);
int csgpu_solve_many_allowed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_options *options,
                             csgpu_many_result *d_results, int32_t *d_solutions, void *stream);
int csgpu_solve_many_allowed_upto(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                  const csgpu_many_upto_options *options, csgpu_many_result *d_results, int32_t *d_solutions,
                                  void *stream);

/* ---- the allowed walk in slices, and its stopped ALL walks spread over the next launch ----
 * csgpu_solve_many_allowed_checkpointed / _resume and csgpu_solve_many_allowed_upto_checkpointed / _upto_resume are to the
 * two calls above what csgpu_solve_many_checkpointed / _resume and csgpu_solve_many_upto_checkpointed / _upto_resume are to
 * csgpu_solve_many / _upto.  The pool is csgpu_many_checkpoints_create's; slot bytes, reset and free are unchanged, and a
 * frame is the walk's own {row, variable, next}: the current node is kept with next = the allowed value the walk would try
 * next, and a resume rebuilds allowed(variable) on it and drops the values below next, as coming back to a frame does.
 * d_slots: as in the width calls, word for word -- [count], written by the checkpointed call and read by the resume;
 * -1 = no checkpoint (DONE, BAD_ROOT, or LIMIT while the pool was empty, which then ends exactly as the plain allowed
 * call); a resumed instance goes back into the same slot.  max_nodes is the budget of THIS call; counters accumulate; the
 * first solution, or under up-to-k row index `solutions`, goes on where it was, so a walk in slices is, field for field and
 * row for row, the plain allowed call with the summed budget.  A resumed up-to-k instance whose record already holds
 * max_solutions solutions ends DONE before it tries a node.
 * A slot written by these calls carries a magic of its own: the two walks are different trees with different counters.
 * csgpu_solve_many_resume / _upto_resume on an allowed slot, and the allowed resumes on a width slot, a free slot or a
 * slot >= capacity, give CSGPU_MANY_BAD_SLOT with nothing else of the instance touched; csgpu_many_checkpoint_children
 * counts -1 for an allowed slot and csgpu_many_checkpoint_fanout writes nothing for it.
 * csgpu_many_checkpoint_states accepts the slots of both walks: [next, hi] of every frame is a correct cover of an allowed
 * walk's open subtrees for a csgpu_search, which cuts the forbidden values itself.  The solutions are the walk's; the
 * counters of such a finish are the engine's, not this walk's.
 * csgpu_many_allowed_checkpoint_children / _fanout are csgpu_many_checkpoint_children / _fanout for allowed slots: the
 * untried children of frame d are the values c in [next, hi(variable)] of the frame's row that no valued variable of that
 * row forbids, ascending, frames from `depth` down to 0; a child row is the frame's row in absolute bounds with variable =
 * [c, c], d_owner[row] = i.  -1 for a refused slot (the checks of the width count, with the allowed magic), nothing
 * written unless d_offsets[i + 1] - d_offsets[i] is the count and the rows lie inside [0, total).  The sub-instances are
 * walked by csgpu_solve_many_allowed_checkpointed under ALL and folded by csgpu_many_fold, unchanged.  The split is exact
 * for the reason it is exact on the width walk: the allowed sets are a function of the node's row and the model's table
 * only; the fixpoint of a != network is unique, so the root node of a child row is the child's fixpoint and the sub-walk
 * is the subtree; hence nodes += 1 + sub.nodes, cuts += sub.cuts + (inconsistent as a root), props += sub.root_props +
 * sub.props, solutions += sub.solutions.  A forbidden value is no child row: the walk does not count it either.
 * Errors before any HIP call, in order, are those of the corresponding width entry; in addition the root domain of more
 * than 128 values -> CSGPU_E_LIMIT of the allowed family (for the two fan-out calls after those of
 * csgpu_many_checkpoint_children / _fanout, a clause-kind pool -> CSGPU_E_ARG included).  "One call in flight per model"
 * covers these calls; calls of all families may be queued behind each other on one stream. */
int csgpu_solve_many_allowed_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                          const csgpu_many_options *options, csgpu_many_result *d_results, int32_t *d_solutions,
                                          csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_solve_many_allowed_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options,
                                    csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck,
                                    int32_t *d_slots, void *stream);
int csgpu_solve_many_allowed_upto_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                               const csgpu_many_upto_options *options, csgpu_many_result *d_results,
                                               int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_solve_many_allowed_upto_resume(const csgpu_model *m, int64_t count, const csgpu_many_upto_options *options,
                                         csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck,
                                         int32_t *d_slots, void *stream);
int csgpu_many_allowed_checkpoint_children(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                           int64_t *d_children, void *stream);
int csgpu_many_allowed_checkpoint_fanout(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                         const int64_t *d_offsets, csgpu_val *d_rows, int32_t *d_owner, int64_t total,
                                         void *stream);

/* ---- Luby restarts with a seeded value order, for ANY: csgpu_solve_many whose deep walks are cut short ----
 * The deep instances of a batch are the heavy tail of a depth-first search with a fixed value order.  This call walks
 * the ANY walk of csgpu_solve_many with two changes, both per instance; everything not mentioned (the root check and
 * BAD_ROOT, the root node, the branching rule, the counters and props, the budget compared before a child is tried, at
 * most n_vars - 1 frames) is csgpu_solve_many's.  State: run = 0, fails = 0, Luby state threshold = 1, counter = 1
 * (csgpu_luby_next).
 *   value order   a node that branches on variable v with the interval [lo, hi], width = hi - lo + 1, tries
 *                 value(j) = lo + ((start + j) mod width) for j = 0 .. width - 1.  start = 0 when run == 0 and
 *                 CSGPU_MANY_ROTATE_FIRST is not set; otherwise start = (uint64_t)key * width >> 32 with
 *                 key = fmix32(seed_i ^ fmix32(run * 0x9E3779B1u + (uint32_t)v + 1u)), all in wrapping uint32_t, and
 *                 fmix32(x): x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16.
 *                 seed_i = d_seeds[i], or options->seed for every instance when d_seeds is NULL: an instance's answer
 *                 depends on its row, its seed and the options, not on its position in the batch.  start is computed
 *                 once per entered node (and again when a node comes back from its frame, which holds {v, next j}).
 *   restart       after a child fails and the cut is counted: if it was the node's last value and no frame is left,
 *                 this run has walked the whole tree -- DONE with 0 solutions, proven, no restart.  Otherwise, when
 *                 restart_base > 0: fails++, and if fails > threshold * restart_base (in 64 bits): fails = 0,
 *                 csgpu_luby_next(&threshold, &counter), run++, restarts++, and the walk starts again from the root
 *                 node's fixpoint at depth 0, the branching variable selected anew, j = 0.  A restart costs no node;
 *                 root_props is counted once; nodes / cuts / props accumulate over the runs and max_nodes is their
 *                 total.  Thresholds grow without bound, so an instance without a solution is still proven so.
 * restart_base = 0 with flags 0 is csgpu_solve_many under ANY, field for field and row for row, and so is every instance
 * whose first run ends before its first restart.  restart_base = 0 with CSGPU_MANY_ROTATE_FIRST is one seeded walk (a
 * sampler of solutions; it has the heavy tail).  There are no checkpoints: the walk is deterministic, an instance that
 * ends LIMIT can be run again with a larger budget.
 *   d_seeds       NULL, or [count] uint32
 *   d_solutions   NULL, or [count][n_vars] int32: the solution of an instance that found one, else not touched
 *   d_restarts    NULL, or [count] int32: the restarts of every instance (0 for a BAD_ROOT row)
 * The call uses the model's workspace and ticket counters like the calls above: one call in flight per model, calls of
 * all families may be queued behind each other on one stream without the host in between.
 * Errors before any HIP call, in csgpu_solve_many's order: a null model / roots / results / options, count < 0,
 * max_nodes <= 0, restart_base < 0, a flag bit other than CSGPU_MANY_ROTATE_FIRST -> CSGPU_E_ARG; model not finalized ->
 * CSGPU_E_STATE; model does not qualify for kernel 7 -> CSGPU_E_LIMIT.  count == 0 -> CSGPU_OK, nothing is launched. */
#define CSGPU_MANY_ROTATE_FIRST 1
typedef struct csgpu_many_restart_options {
  int64_t max_nodes;     /* > 0, over all runs of an instance */
  int64_t restart_base;  /* >= 0; 0: no restarts */
  uint32_t seed;         /* used where d_seeds is NULL */
  int32_t flags;         /* 0 or CSGPU_MANY_ROTATE_FIRST; any other bit: CSGPU_E_ARG */
} csgpu_many_restart_options;   /* 24 bytes */
int csgpu_solve_many_restarts(const csgpu_model *m, const csgpu_val *d_roots, const uint32_t *d_seeds, int64_t count,
                              const csgpu_many_restart_options *options, csgpu_many_result *d_results,
                              int32_t *d_solutions /* NULL or [count][n_vars] */, int32_t *d_restarts /* NULL or [count] */,
                              void *stream);
/* host, no device: the value a node tries j-th -- the definition above, exported so it can be pinned (j is taken mod
 * width) */
int32_t csgpu_many_value(uint32_t seed, uint32_t run, int32_t var, csgpu_val bounds, uint32_t j, int32_t flags);

/* ---- every solution of every instance under ALL: csgpu_solve_many whose solutions go to one bounded stream ----
 * csgpu_solve_many under ALL counts an instance's solutions and keeps the first; csgpu_solve_many_upto keeps k rows per
 * instance, k chosen in advance.  This call enumerates: the walk is csgpu_solve_many's ALL walk unchanged (the root check
 * and BAD_ROOT, the root node, the branching rule, ascending values, the counters, the budget compared before a child is
 * tried), and every solution is appended to ONE output stream that all instances share.  options->objective must be 1;
 * options->max_nodes is the budget of THIS call per instance (nodes tried in the call), as in csgpu_solve_many_resume.
 * One entry point starts and resumes instances, because with a bounded stream every call after the first does both.
 *   appending     when a child, or the root node, has every variable valued, one relaxed agent-scope atomic adds 1 to
 *                 *d_count; the old value idx is the row.  idx < capacity: d_rows[idx] receives the solution (absolute
 *                 values), d_owner[idx] the instance, and the solution is counted.  idx >= capacity: it is refused (below).
 *                 The kernel never zeroes *d_count: after a call the valid rows are the first min(*d_count, capacity), and
 *                 the caller copies them out and zeroes the word on the same stream before the next call.  One wave walks
 *                 an instance at a time and calls are ordered on the stream, so the rows of one instance appear in walk
 *                 order: by index within a call, by call across calls.
 *   refusal       a refused solution is not lost.  The child that produced it is not counted (nodes, cuts, props and
 *                 solutions are what they were before it was tried), the instance stops with CSGPU_MANY_FULL, and its
 *                 checkpoint stands at "try value nv of variable bv on this node" with nv that very value, in the slot
 *                 layout above.  The next call tries the child again, and it is counted once.
 *   d_slots[i]    on entry  -2 (CSGPU_MANY_SLOT_FRESH): start instance i from root row i.  -1, or anything below -2:
 *                 finished, nothing of the instance is read or written.  >= 0: go on from that slot, the counters are read
 *                 from d_results[i]; a number outside the pool, or a slot without a checkpoint, gives CSGPU_MANY_BAD_SLOT,
 *                 compared before anything is read, and nothing else is touched.
 *                 on exit   -2: not started -- the wave that drew it found the stream full already, or its root row is
 *                 itself the solution and found no room; status FULL, the other fields zero.  -1: finished (DONE,
 *                 BAD_ROOT), or stopped (LIMIT / FULL, with its counters) while the pool had no slot left: its walk is gone,
 *                 exactly as in csgpu_solve_many_checkpointed.  >= 0: stopped with a checkpoint (LIMIT or FULL); a resumed
 *                 instance goes back into the SAME slot.
 *   full at the draw   a wave that has drawn a ticket first reads *d_count (relaxed); if it is >= capacity already the
 *                 wave does not walk: a fresh instance stays -2 with status FULL, one with a slot is left exactly as it
 *                 was.  So a full stream drains the remaining tickets quickly.
 * The caller's loop:  slots = -2; do { call; take the rows; zero the count } while (any slot != -1).  A pool of `count`
 * slots never runs out, and with such a pool every instance ends DONE with its record equal, field for field, to
 * csgpu_solve_many under ALL with an unlimited budget, whatever capacity >= 1 and budget the calls had; the rows drained for
 * the instance are its walk's solutions in walk order, each exactly once.
 * The pool is that of csgpu_many_checkpoints_create with its slot layout; csgpu_many_checkpoint_states works unchanged on a
 * slot written here.  "One call in flight per model" covers this call (same workspace, same ticket counters); calls of
 * all families may be queued behind each other on one stream without the host in between.
 * Errors before any HIP call, in csgpu_solve_many's order: a null m / d_roots / d_results / options / ck / d_slots / out,
 * count < 0, max_nodes <= 0 -> CSGPU_E_ARG; an objective other than ALL -> CSGPU_E_ARG; capacity < 1 or a null pointer
 * inside *out -> CSGPU_E_ARG; model not finalized -> CSGPU_E_STATE; model does not qualify for kernel 7 -> CSGPU_E_LIMIT; a
 * pool of another model or of the clause kind -> CSGPU_E_ARG; count > 2^31 - 65 -> CSGPU_E_LIMIT.  count == 0 -> CSGPU_OK,
 * nothing is launched. */
#define CSGPU_MANY_FULL 4          /* stopped because the solution stream had no room */
#define CSGPU_MANY_SLOT_FRESH (-2) /* d_slots[i] on entry: start instance i from its root row */
typedef struct csgpu_many_stream {
  int32_t  *d_rows;   /* [capacity][n_vars]: the solutions, absolute values */
  int32_t  *d_owner;  /* [capacity]: the instance a row belongs to */
  uint64_t *d_count;  /* ONE device word: append attempts since the caller last zeroed it */
  int64_t   capacity; /* >= 1 */
} csgpu_many_stream;   /* 32 bytes; caller-owned device memory */
int csgpu_solve_many_stream(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_options *options,
                            csgpu_many_result *d_results, csgpu_many_checkpoints *ck, int32_t *d_slots,
                            const csgpu_many_stream *out, void *stream);

/* ---- many instances of one CLAUSE model in one call: a depth-first search per wavefront, also under MIN / MAX ----
 * csgpu_solve_many for the models it refuses: `=`, `<`, disjunctions, expression trees, an objective -- the scheduling
 * models with other release times, windows or deadlines per row.  Built on kernel 6 (csgpu_model_qualifies(m, 6): at
 * most 512 clauses, resident in registers).  csgpu_many_options and csgpu_many_result are those of csgpu_solve_many;
 * options->objective also takes 2 MIN and 3 MAX, on this entry only.
 *
 * The walk.  One wavefront takes an instance from its root row to its answer.
 *   Root.       A row with lo > hi, or outside the model's root domains, gives CSGPU_MANY_BAD_ROOT and is not searched.
 *               Otherwise the root node runs, a `var < 0` node of kernel 6: rounds over all clauses until nothing
 *               changes.  An inconsistent root gives CSGPU_MANY_DONE with 0 nodes.  A root with every variable valued is
 *               the one solution.
 *   Branching.  The branching variable is the open variable with the smallest hi - lo, ties to the lowest index, over
 *               all variables including "<obj>".  Values are tried in ascending order.  A child is the assignment
 *               followed by the fixpoint.  A consistent child with open variables is entered at once; its parent is
 *               pushed only if it has values left.  max_nodes is compared before a child is tried.
 *   Counters.   nodes = children tried, cuts = inconsistent children, solutions = children with every variable valued,
 *               props / root_props = kernel 6's props of the consistent children / of the root.
 *   MIN / MAX.  Each instance has a private incumbent, none at the start, so its tree is deterministic.  Before a
 *               child's fixpoint, and only once the instance has a solution, dom[obj] becomes the objective bound of
 *               csgpu_objective_bound(objective, dom[obj], best): what kernel 6 does at node entry, so a frame popped
 *               from the stack is bounded again when its next child is made.  If the bound empties dom[obj], the child
 *               is a node and a cut.  A solution sets best to "<obj>"'s value and overwrites the instance's row in
 *               d_solutions; the search goes on to the end of the tree.  CSGPU_MANY_DONE means the optimum is proven, or
 *               that there is no solution.  CSGPU_MANY_LIMIT leaves the best found so far in d_best and d_solutions: an
 *               anytime answer.
 *   ANY / ALL.  Exactly csgpu_solve_many's meaning: ANY leaves at the first solution, and the row stored is the first
 *               solution.  The model's "<obj>" variable, if it has one, is then an ordinary variable.
 *   d_best      NULL, or [count] int32: written only for instances with at least one solution under MIN / MAX.
 * Which models qualify (csgpu_model_qualifies_many_clauses): finalized, kernel 6 planned, and the per-wave LDS slice
 * (n_vars * 8 + 16 bytes) times the four waves of a workgroup fits the 160 KiB of a CU.
 * Workspace and tickets are the model's, shared with csgpu_solve_many: ONE call of the whole family in flight per
 * model; a call may be queued behind another on the same stream without the host in between.  A frame holds absolute
 * bounds; a wave has n_vars frames of (n_vars + 1) x 8 bytes, and a call launches min(count, resident waves) waves, fewer
 * where their frames would pass 1 GiB.
 * Errors before any HIP call, in csgpu_solve_many's order: null model / roots / results / options, count < 0,
 * max_nodes <= 0 -> CSGPU_E_ARG; an objective other than 0-3, MIN / MAX on a model without an objective variable or
 * with the other sense -> CSGPU_E_ARG; model not finalized -> CSGPU_E_STATE; more than 512 clauses, or slices that do
 * not fit -> CSGPU_E_LIMIT, the message says which; count > 2^31 - 65 -> CSGPU_E_LIMIT.  count == 0 -> CSGPU_OK, nothing
 * is launched.
 * An instance that stops at max_nodes need not start again from its root row: see "clause checkpoints" below. */
int csgpu_model_qualifies_many_clauses(const csgpu_model *m);
int csgpu_solve_many_clauses(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_options *options,
                             csgpu_many_result *d_results, int32_t *d_solutions /* NULL or [count][n_vars] */,
                             int32_t *d_best /* NULL or [count] */, void *stream);

/* ---- clause checkpoints: csgpu_solve_many_clauses in slices ----
 * What "checkpoints: csgpu_solve_many in slices" above is to csgpu_solve_many, for csgpu_solve_many_clauses, MIN / MAX
 * included: an instance that stops at max_nodes with work left draws a slot of a pool and leaves there its pushed frames,
 * its current node with {branching variable, next value}, and its incumbent.  The bound of a stopped MIN / MAX walk is
 * what makes the rest of its tree small; it goes on with it.
 *   csgpu_many_clause_checkpoints_create   a pool for these calls.  The type, csgpu_many_checkpoints_reset and
 *                                  csgpu_many_checkpoints_free are those above; a pool remembers its kind, and every
 *                                  call of either family answers CSGPU_E_ARG to a pool of the other kind
 *   csgpu_solve_many_clauses_checkpointed   csgpu_solve_many_clauses plus the pool: d_slots[i] receives the slot of an
 *                                  instance that stopped with a checkpoint and -1 for every other one (DONE, BAD_ROOT, or
 *                                  LIMIT while the pool had no slot left: such an instance ends exactly as in
 *                                  csgpu_solve_many_clauses)
 *   csgpu_solve_many_clauses_resume   the same d_results / d_solutions / d_best / d_slots rows again, options->max_nodes
 *                                  being the budget of THIS call (nodes tried in the call).  An instance with
 *                                  d_slots[i] < 0 is left untouched: nothing of it is written.  One with a slot reads its
 *                                  counters from d_results[i] and its incumbent from the slot, goes on in the slot's
 *                                  frames, and ends DONE (d_slots[i] = -1) or LIMIT (header and {variable, next value}
 *                                  go back into the SAME slot).  Counters accumulate; under MIN / MAX d_solutions /
 *                                  d_best are overwritten at every improvement, under ANY / ALL the row is stored when
 *                                  `solutions` becomes 1.  A walk in slices gives, field for field and row for row, the
 *                                  one csgpu_solve_many_clauses call with the summed budget
 *   csgpu_many_clause_checkpoint_states   the open subtrees of one checkpoint as states, the oldest frame (the largest
 *                                  subtree) first: a frame {row, bv, next} becomes the row with bv narrowed to
 *                                  [next, row[bv].hi], the current node likewise.  *count = depth + 1; *have_best and
 *                                  *best are the incumbent.  The states are NOT at the fixpoint yet, and the incumbent's
 *                                  bound is not in them: run them through csgpu_propagate_batch_obj as `var < 0` nodes
 *                                  under the bound, drop the inconsistent ones and count the complete ones, then
 *                                  csgpu_search_set_best and csgpu_search_put.  Errors as csgpu_many_checkpoint_states
 *                                  (best / have_best must not be null); it reads the header on `stream` and waits
 * The kernel gives CSGPU_MANY_BAD_SLOT, with nothing but the status word written, to an instance whose slot number is
 * outside [0, capacity), whose slot holds no checkpoint (the magic word is missing or the depth is outside [0, n_vars)),
 * or whose checkpoint was made under another objective than options->objective.  All of that is compared before
 * anything else of the slot is read.
 * A slot is csgpu_many_clause_checkpoint_bytes(m) bytes: (n_vars + 1) frames of (n_vars + 1) 8-byte entries in absolute
 * bounds.  Frame 0 is the header: entry 0 {depth, magic}, entry 1 {best, have_best | objective << 1} (4 in place of the
 * objective: a checkpoint of csgpu_solve_many_clauses_upto_checkpointed, below).  Frames 1 .. depth
 * are the pushed frames, the row and then {variable, next value}; frame 1 + depth is the current node as it was entered,
 * with {variable, next value} behind it.  Slots are freed by csgpu_many_checkpoints_reset only.
 * Concurrency: ONE call of the whole csgpu_solve_many family in flight per model, as before; calls may be queued on one
 * stream without the host in between (a checkpointed call and its resumes, for instance).  The same slot number twice in
 * one resume call is undefined.  The pool outlives the calls queued on it and is freed before its model.
 * Errors before any HIP call, in csgpu_solve_many_clauses's order and with its codes; after them a null pool or d_slots,
 * a pool created for another model, a pool of csgpu_many_checkpoints_create -> CSGPU_E_ARG; then count == 0 -> CSGPU_OK,
 * nothing is launched.  csgpu_many_clause_checkpoints_create: as csgpu_many_checkpoints_create, CSGPU_E_LIMIT for a
 * model that does not qualify for csgpu_solve_many_clauses.
 * This note used to read "Not here: restarts for clause models", and before that "Not here: up to k solutions and restarts
 * for clause models": both halves are closed, up to k solutions are the next section and restarts the one after it. */
size_t csgpu_many_clause_checkpoint_bytes(const csgpu_model *m); /* bytes per slot; 0 if the model does not qualify (at most
                                                                    512 clauses, slices that fit), and for NULL.  No HIP
                                                                    call: after finalize, or after
                                                                    csgpu_model_build_tables alone */
int csgpu_many_clause_checkpoints_create(const csgpu_model *m, int64_t capacity, csgpu_many_checkpoints **out);
int csgpu_solve_many_clauses_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                          const csgpu_many_options *options, csgpu_many_result *d_results, int32_t *d_solutions,
                                          int32_t *d_best, csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_solve_many_clauses_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options,
                                    csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                    csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_many_clause_checkpoint_states(const csgpu_many_checkpoints *ck, int32_t slot, csgpu_val *d_states, int64_t cap,
                                        int64_t *count, int32_t *best, int32_t *have_best, void *stream);

/* ---- stopped ALL walks of a clause model spread over the waves of the next call ----
 * What "stopped ALL walks spread over the waves of the next call" above is to csgpu_solve_many, for the clause models, whose
 * batches are the most uneven and the smallest: a call launches at most the resident waves.  A clause checkpoint is the
 * same list of frames "node, branching variable bv, next value" (frame 0 of the slot is the header, frames 1 .. 1 + depth
 * the pushed frames and then the current node), and the walk's untried children are, in WALK ORDER, the values next ..
 * hi(bv) of the current node (ascending), then those of the frame below it, down to the oldest frame.  Each child -- the
 * frame's node, in the absolute bounds it is stored in, with bv = [v, v] -- is a root row that
 * csgpu_solve_many_clauses[_checkpointed] walks like any other: the kernel runs a root row and a child through the same
 * rounds, and under ALL no incumbent narrows the node.  Its record gives its owner exactly the contribution stated above
 * (nodes 1 + sub.nodes; cuts sub.cuts, plus 1 for a row inconsistent as a root; props sub.root_props + sub.props;
 * solutions), and csgpu_many_fold, which reads records and owners only, is SHARED by the two families.
 * These two calls are ALL only.  Under MIN / MAX an instance's incumbent is sequential: a subtree walked without the bound
 * of the one before it is another tree (the same optimum all the same: "start incumbents" below spreads such walks by calls
 * of their own).  So a checkpoint whose header code is not ALL's 1 -- ANY 0, MIN 2, MAX 3, up-to-k 4, the stream 5 --
 * is refused like a slot without a checkpoint.
 *   csgpu_many_clause_checkpoint_children   d_children[i] = the children of the checkpoint in slot d_slots[i] (int64
 *                                    [count], a frame's count is taken in 64 bits: a domain may be 2^32 wide): 0 for
 *                                    d_slots[i] < 0; -1 for a slot that is refused: a number >= capacity, a header
 *                                    without a clause checkpoint, with a depth outside [0, n_vars) or with another code
 *                                    than ALL's, a frame whose variable is outside [0, n_vars), whose node's bounds of it
 *                                    lie outside the model's root domain or are empty, or whose next value lies outside
 *                                    those bounds.  Everything is compared before what depends on it is read
 *   csgpu_many_clause_checkpoint_fanout     as csgpu_many_checkpoint_fanout: d_offsets int64 [count + 1] on the device,
 *                                    rows in walk order to d_rows ([total][n_vars]), d_owner[row] = i if d_owner is not
 *                                    NULL; the slot is counted again first and NOTHING is written unless d_offsets[i + 1]
 *                                    - d_offsets[i] is that count and the rows lie inside [0, total).  The rows are copies
 * Both are asynchronous on `stream`, read the pool only, use no atomics, and take a pool of
 * csgpu_many_clause_checkpoints_create.  Errors before any HIP call, in this order: a null pointer (d_owner may be null) ->
 * CSGPU_E_ARG; count < 0 or total < 0 -> CSGPU_E_ARG; a pool of csgpu_many_checkpoints_create -> CSGPU_E_ARG; count >
 * 2^31 - 1 -> CSGPU_E_LIMIT.  Then count == 0 or total == 0 -> CSGPU_OK, nothing is launched. */
int csgpu_many_clause_checkpoint_children(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                          int64_t *d_children, void *stream);
int csgpu_many_clause_checkpoint_fanout(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                        const int64_t *d_offsets, csgpu_val *d_rows, int32_t *d_owner, int64_t total, void *stream);

/* ---- start incumbents, and stopped MIN / MAX walks of a clause model spread over the waves of the next call ----
 * The sequential incumbent above only matters if a split has to reproduce the one call's TREE.  It does not matter for the
 * OPTIMUM: a stopped MIN / MAX walk's untried children are independent sub-problems, and any known solution value is a
 * valid bound for all of them.  The primitive is an instance that starts its walk with an incumbent it did not find
 * itself; it also serves as a warm start (a row with a known upper bound) and for "prove that nothing beats 45".
 * The walk (kernel cs_walk_from) is csgpu_solve_many_clauses's under MIN / MAX -- same root check, branching rule, value
 * order, counters and budget -- with three differences:
 *   starting      a fresh instance i with d_start[i].have != 0 begins with have_best = true, best = d_start[i].best: dom[obj]
 *                 of its root row becomes csgpu_objective_bound(objective, dom[obj], best) before the root node's rounds, as
 *                 a child's does once the instance has a solution.  A bound that empties dom[obj] makes the root node
 *                 inconsistent: DONE, 0 nodes, 0 solutions.  have == 0 gives the walk of csgpu_solve_many_clauses
 *                 [_checkpointed], field for field and row for row (`best` is then not read)
 *   own solutions d_best[i] and row i of d_solutions are written only for solutions the instance found itself: d_best iff
 *                 solutions > 0 (the record's count included for a resumed instance).  Every such solution is strictly
 *                 better than the start.  An instance that proves that nothing beats its start ends DONE with solutions ==
 *                 0, its d_best and its row untouched
 *   resuming      a checkpoint's header carries {best, have_best | objective << 1} as every MIN / MAX checkpoint does, the
 *                 start's value included.  csgpu_solve_many_clauses_resume continues such an instance without change (it
 *                 writes d_best whenever the header has an incumbent); csgpu_solve_many_clauses_from_resume continues it
 *                 under the own-solutions rule.  A checkpoint of either MIN / MAX call may be resumed by either resume
 *   csgpu_solve_many_clauses_from         d_start [count] is required; ck == NULL and d_slots == NULL: no checkpoints (the
 *                                         plain call), both given: the checkpointed call
 *   csgpu_solve_many_clauses_from_resume  as csgpu_solve_many_clauses_resume
 * Errors before any HIP call: those of csgpu_solve_many_clauses, in its order and with its codes; then a null d_start, an
 * objective ANY / ALL, exactly one of ck / d_slots null (the resume: either) -> CSGPU_E_ARG; then the pool's errors of
 * csgpu_solve_many_clauses_checkpointed; then count == 0 -> CSGPU_OK.
 *
 * The spread.  csgpu_many_clause_checkpoint_children_obj / _fanout_obj are the two calls above for checkpoints whose
 * header code is `objective` (MIN 2 or MAX 3; anything else -> CSGPU_E_ARG, before the other errors, which are the same):
 * every comparison-before-read rule holds, a slot with another code (an ALL one among them) is -1.  The fan-out writes,
 * beside each row, d_start[row]: the better -- strictly, by csgpu_objective_better's order -- of the slot's header
 * incumbent and d_owner_start[i] (NULL, or [count]; have == 0: none); have == 0 when neither exists.  d_start is required.
 * Nothing is written unless the counted children match the offsets.  The rows are walked by
 * csgpu_solve_many_clauses_from; each sub-instance is deterministic; its counters fold with the unchanged csgpu_many_fold
 * (a sub-row whose start bound emptied dom[obj] is "inconsistent as a root": the +1 cut), and the owner is DONE with the
 * proven optimum when all its sub-instances are DONE.  The walk that was made is larger than the one call's: the optimum
 * is the one call's, the counters are not.
 *   csgpu_many_fold_best   d_key is uint64 [owners], set to all ones by the caller.  For every row t < total with
 *                          d_owner[t] >= 0 and d_sub_results[t].solutions > 0: one relaxed agent-scope 64-bit unsigned min
 *                          of csgpu_many_best_key(objective, d_sub_best[t], t) into d_key[d_owner[t]].  Afterwards a key is
 *                          all ones (nothing found) or names the owner's best value in the batch and the LOWEST row that
 *                          holds it.  Errors: a null pointer, total < 0, an objective other than MIN / MAX -> CSGPU_E_ARG;
 *                          total >= 2^32 -> CSGPU_E_LIMIT; then total == 0 -> CSGPU_OK
 *   csgpu_many_best_key    (rank(best) << 32) | row on the host: rank is the order-preserving map of int32 to uint32 (the
 *                          sign bit flipped) for MIN and its complement for MAX
 *   csgpu_many_key_decode  0 for all ones; else 1, with *best and *row (either may be NULL) */
typedef struct csgpu_many_start {
  int32_t best; /* counts only where have != 0 */
  int32_t have;
} csgpu_many_start;
int csgpu_solve_many_clauses_from(const csgpu_model *m, const csgpu_val *d_roots, const csgpu_many_start *d_start, int64_t count,
                                  const csgpu_many_options *options, csgpu_many_result *d_results, int32_t *d_solutions,
                                  int32_t *d_best, csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_solve_many_clauses_from_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options,
                                         csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                         csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_many_clause_checkpoint_children_obj(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                              int objective, int64_t *d_children, void *stream);
int csgpu_many_clause_checkpoint_fanout_obj(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count, int objective,
                                            const csgpu_many_start *d_owner_start, const int64_t *d_offsets, csgpu_val *d_rows,
                                            int32_t *d_owner, csgpu_many_start *d_start, int64_t total, void *stream);
int csgpu_many_fold_best(const csgpu_many_result *d_sub_results, const int32_t *d_sub_best, const int32_t *d_owner, int64_t total,
                         int objective, uint64_t *d_key, void *stream);
uint64_t csgpu_many_best_key(int objective, int32_t best, uint32_t row);
int csgpu_many_key_decode(int objective, uint64_t key, int32_t *best, uint32_t *row);

/* ---- up to k solutions per instance of a clause model: csgpu_solve_many_clauses, left at the k-th solution ----
 * "Which of these 10,000 schedule rows have a unique timetable?", "three alternatives per row": what "up to k solutions
 * per instance" above is to csgpu_solve_many, for the clause models.  The instance walks exactly the ALL walk of
 * csgpu_solve_many_clauses ("The walk" above: same root check, branching rule, value order and counters; "<obj>", if the
 * model has one, is an ordinary variable and there is no incumbent) and stops right after accepting its k-th solution,
 * as ANY stops after its first.  max_solutions = 1 is ANY, field for field and row for row; an instance whose whole tree
 * holds fewer than k solutions ends as under ALL, field for field.  options is csgpu_many_upto_options and d_results
 * csgpu_many_result, both as above.  CSGPU_MANY_DONE: the k-th solution was reached or the tree is exhausted, and
 * solutions == min(k, solutions of the tree) -- with k = 2, "unique" is DONE && solutions == 1, "several" DONE &&
 * solutions == 2, "none" DONE && solutions == 0.  LIMIT, BAD_ROOT and BAD_SLOT are as above.
 *   d_solutions   NULL, or [count][max_solutions][n_vars] int32: row j of instance i is its j-th solution in walk order
 *                 (a root row that is a solution already is row 0); rows >= solutions of an instance are not touched.
 *                 count * max_solutions * n_vars may pass 2^31: the rows are indexed in 64 bits
 * The three entries are csgpu_solve_many_clauses, csgpu_solve_many_clauses_checkpointed and
 * csgpu_solve_many_clauses_resume with this stop.  The pool is one of csgpu_many_clause_checkpoints_create; slots, their
 * layout, csgpu_many_clause_checkpoint_states (*have_best is 0) and csgpu_many_checkpoints_reset are those of "clause
 * checkpoints", unchanged.  The header's code field (have_best | code << 1) holds 4, "up to k", where the other calls
 * write their objective 0 .. 3: a checkpoint made here gives CSGPU_MANY_BAD_SLOT to csgpu_solve_many_clauses_resume
 * under any objective, and one made there gives it to csgpu_solve_many_clauses_upto_resume, compared before anything
 * else of the slot is read and with nothing but the status word written.  A resumed instance reads its counters from its
 * record and continues its rows at index `solutions`: a walk in slices gives, field for field and row for row, the one
 * call with the summed budget.  max_solutions is per call: a resumed instance whose record already has solutions >=
 * max_solutions ends DONE before it tries a node, and nothing of it is written but its status and d_slots[i] = -1 (rows
 * are indexed with the max_solutions of the call that writes them: give every slice the k the buffer was laid out for, or
 * a buffer laid out for the new k).  ONE call of the whole csgpu_solve_many family in flight per model (same workspace,
 * same ticket counters); calls of all families may be queued behind each other on one stream without the host in
 * between.
 * Errors before any HIP call, in csgpu_solve_many_clauses's order and with its codes: null model / roots / results /
 * options (d_solutions may be null), count < 0, max_nodes <= 0, max_solutions < 1 -> CSGPU_E_ARG; model not finalized ->
 * CSGPU_E_STATE; more than 512 clauses, or slices that do not fit -> CSGPU_E_LIMIT; count > 2^31 - 65 -> CSGPU_E_LIMIT;
 * the checkpointed and the resume entry: a null pool or d_slots, a pool created for another model, a pool of
 * csgpu_many_checkpoints_create -> CSGPU_E_ARG; then count == 0 -> CSGPU_OK, nothing is launched. */
int csgpu_solve_many_clauses_upto(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                  const csgpu_many_upto_options *options, csgpu_many_result *d_results,
                                  int32_t *d_solutions /* NULL or [count][max_solutions][n_vars] */, void *stream);
int csgpu_solve_many_clauses_upto_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                               const csgpu_many_upto_options *options, csgpu_many_result *d_results,
                                               int32_t *d_solutions, csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_solve_many_clauses_upto_resume(const csgpu_model *m, int64_t count, const csgpu_many_upto_options *options,
                                         csgpu_many_result *d_results, int32_t *d_solutions, csgpu_many_checkpoints *ck,
                                         int32_t *d_slots, void *stream);

/* ---- Luby restarts with a seeded value order for ANY instances of a clause model ----
 * What "Luby restarts with a seeded value order, for ANY" above is to csgpu_solve_many, for the clause models: the deep
 * instances of a batch of schedule rows are the heavy tail of a fixed ascending value order.  The walk is
 * csgpu_solve_many_clauses under ANY ("The walk" above) with exactly the two changes of csgpu_solve_many_restarts, per
 * instance.  State: run = 0, fails = 0, Luby state threshold = 1, counter = 1 (csgpu_luby_next).
 *   value order   a node that branches on variable v with [lo, hi] tries
 *                 csgpu_many_value(seed_i, run, v, {lo, hi}, j, flags) for j = 0 .. hi - lo: the rotation
 *                 lo + ((start + j) mod width) defined above, its width-0 case included.  start = 0 in run 0 unless
 *                 CSGPU_MANY_ROTATE_FIRST is set.  seed_i = d_seeds[i], or options->seed where d_seeds is NULL.  A
 *                 frame's 8-byte entry holds {variable, next j}, not {variable, next value}; `last` is j == hi - lo of
 *                 the node as it was entered.
 *   restart       after a child fails and the cut is counted: if it was the node's last value and no frame is pushed
 *                 (last && depth == 0): DONE with 0 solutions, proven, no restart.  Otherwise, when restart_base > 0:
 *                 fails++, and if fails > threshold * restart_base (in 64 bits): fails = 0,
 *                 csgpu_luby_next(&threshold, &counter), run++, restarts++, and the walk starts again from the root
 *                 node's fixpoint at depth 0, the branching variable selected anew, j = 0.  No node is counted and no
 *                 rounds are run for it: the stored root is at its fixpoint.  root_props is counted once; nodes, cuts
 *                 and props accumulate over the runs and max_nodes is their total.
 * Everything else is csgpu_solve_many_clauses's under ANY: the root check and BAD_ROOT, an inconsistent or all-valued
 * root, the branching rule, the budget compared before a child is tried, and "<obj>" as an ordinary variable.
 * restart_base = 0 with flags 0 is csgpu_solve_many_clauses under ANY, field for field and row for row, and so is every
 * instance whose first run ends before its first restart.
 * ANY only: under MIN / MAX only a run that walks the whole tree proves anything, and restarts make that proof dearer;
 * ALL and up to k enumerate.  The options struct, csgpu_many_restart_options, cannot express another objective.  There
 * are no checkpoints: the walk is deterministic, an instance that ends LIMIT is run again with a larger budget.
 *   d_seeds       NULL, or [count] uint32
 *   d_solutions   NULL, or [count][n_vars] int32: the solution of an instance that found one, else not touched
 *   d_restarts    NULL, or [count] int32: the restarts of every instance (0 for a BAD_ROOT row)
 * A wave has n_vars + 1 frames here: the walk's n_vars and one that keeps the root node's fixpoint.  Workspace and
 * tickets are the model's: ONE call of the whole csgpu_solve_many family in flight per model; calls of all families may
 * be queued behind each other on one stream without the host in between.
 * Errors before any HIP call, in the family's order: null model / roots / results / options, count < 0, max_nodes <= 0,
 * restart_base < 0, a flag bit other than CSGPU_MANY_ROTATE_FIRST -> CSGPU_E_ARG; model not finalized -> CSGPU_E_STATE;
 * a model that does not qualify for csgpu_solve_many_clauses, or count > 2^31 - 65 -> CSGPU_E_LIMIT.  count == 0 ->
 * CSGPU_OK, nothing is launched. */
int csgpu_solve_many_clauses_restarts(const csgpu_model *m, const csgpu_val *d_roots, const uint32_t *d_seeds, int64_t count,
                                      const csgpu_many_restart_options *options, csgpu_many_result *d_results,
                                      int32_t *d_solutions /* NULL or [count][n_vars] */,
                                      int32_t *d_restarts /* NULL or [count] */, void *stream);

/* ---- every solution of every instance of a clause model under ALL, through one bounded stream ----
 * What "every solution of every instance under ALL" above is to csgpu_solve_many, for the clause models: "every timetable
 * of these 10,000 windows", where one row has 8 and its neighbour a quarter of a million, so that no k of
 * csgpu_solve_many_clauses_upto fits.  The walk is the ALL walk of csgpu_solve_many_clauses_upto ("The walk" above: same
 * root check and BAD_ROOT, root node, branching rule, ascending values and counters; "<obj>", if the model has one, is an
 * ordinary variable and there is no incumbent, so a model whose own objective is MIN or MAX is accepted), and every
 * solution is appended to ONE output stream that all instances share.  csgpu_many_stream, CSGPU_MANY_FULL and
 * CSGPU_MANY_SLOT_FRESH are those above.  options->objective must be 1; options->max_nodes is the budget of THIS call per
 * instance (nodes tried in the call), as in csgpu_solve_many_clauses_resume; LIMIT behaves as there.  One entry point
 * starts and resumes instances, because with a bounded stream every call after the first does both.
 *   appending     when a child, or the root node after its fixpoint, has every variable valued, one relaxed agent-scope
 *                 atomic adds 1 to *d_count; the old value idx is the row.  idx < capacity: d_rows[idx] receives the
 *                 solution (absolute values, a row index of 64 bits), d_owner[idx] the instance, and the solution is
 *                 counted.  idx >= capacity: it is refused (below).  The kernel never zeroes *d_count: after a call the
 *                 valid rows are the first min(*d_count, capacity), and the caller copies them out and zeroes the word on
 *                 the same stream before the next call.  One wave walks an instance at a time and calls are ordered on the
 *                 stream, so the rows of one instance appear in walk order: by index within a call, by call across calls.
 *   refusal       a refused solution is not lost.  The child that produced it is not counted (nodes, cuts, props and
 *                 solutions are what they were before it was tried), the instance stops with CSGPU_MANY_FULL, and it
 *                 writes the checkpoint a LIMIT stop writes: frames 0 .. depth and {variable, next value} with the next
 *                 value that very value.  The next call tries the child again, and it is counted once.  A root node that
 *                 is itself the solution and finds no room: status FULL, every other field zero, d_slots[i] stays -2, and
 *                 the next call runs the root again.
 *   d_slots[i]    on entry  -2 (CSGPU_MANY_SLOT_FRESH): start instance i from root row i.  -1, or anything below -2:
 *                 finished, nothing of the instance is read or written.  >= 0: go on from that slot, the counters are read
 *                 from d_results[i]; a number outside the pool, a slot without a checkpoint, or one whose header holds
 *                 another code than 5 gives CSGPU_MANY_BAD_SLOT, compared before anything else of the slot is read, and
 *                 only the status is written.
 *                 on exit   -2: not started (see "full at the draw" and the root node above).  -1: finished (DONE,
 *                 BAD_ROOT), or stopped (LIMIT / FULL, with its counters) while the pool had no slot left: its walk is
 *                 gone, as in csgpu_solve_many_clauses_checkpointed, but no row of it is.  >= 0: stopped with a checkpoint
 *                 (LIMIT or FULL); a resumed instance goes back into the SAME slot.
 *   full at the draw   a wave that has drawn a ticket first reads *d_count (relaxed); if it is >= capacity already the
 *                 wave does not walk: a fresh instance stays -2 with status FULL and zero fields, one with a slot is left
 *                 exactly as it was.  So a full stream drains the remaining tickets quickly.
 * The caller's loop:  slots = -2; do { call; take the rows; zero the count } while (any slot != -1).  The guarantee: a
 * pool of `count` slots never runs out, and with such a pool every instance ends DONE with its record equal, field for
 * field, to csgpu_solve_many_clauses under ALL with an unlimited budget, whatever capacity >= 1 and budget the calls had;
 * the rows drained for the instance are its walk's solutions in walk order, each exactly once.
 * The pool is one of csgpu_many_clause_checkpoints_create with its slot layout.  The header's code field holds 5, "stream":
 * a checkpoint made here gives CSGPU_MANY_BAD_SLOT to csgpu_solve_many_clauses_resume and
 * csgpu_solve_many_clauses_upto_resume, and theirs give it here.  csgpu_many_clause_checkpoint_states accepts a slot
 * written here as it accepts an up-to-k one (*have_best is 0).  "One call in flight per model" covers this call (same
 * workspace, sized as for a fresh call, same ticket counters); calls of all families may be queued behind each other on
 * one stream without the host in between.
 * Errors before any HIP call, in csgpu_solve_many_clauses's order: a null m / d_roots / d_results / options / ck /
 * d_slots / out, count < 0, max_nodes <= 0 -> CSGPU_E_ARG; an objective other than ALL -> CSGPU_E_ARG; capacity < 1 or a
 * null pointer inside *out -> CSGPU_E_ARG; model not finalized -> CSGPU_E_STATE; a model that does not qualify for
 * csgpu_solve_many_clauses -> CSGPU_E_LIMIT; count > 2^31 - 65 -> CSGPU_E_LIMIT; a pool of another model or of
 * csgpu_many_checkpoints_create -> CSGPU_E_ARG.  count == 0 -> CSGPU_OK, nothing is launched. */
int csgpu_solve_many_clauses_stream(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                    const csgpu_many_options *options, csgpu_many_result *d_results,
                                    csgpu_many_checkpoints *ck, int32_t *d_slots, const csgpu_many_stream *out, void *stream);

/* ---- the engine's five variable orders and interval halving for the instances of a clause model ----
 * csgpu_solve_many_clauses branches on the smallest interval and tries every value of it: a variable that a row leaves
 * at its root width of 2^31 values is enumerated until the budget runs out.  This entry walks the same walk with the two
 * things the search engine has for that (csgpu_search_set_strategy's orders, and halving of an interval of more than 256
 * values).  csgpu_many_result is csgpu_solve_many's.
 *
 * The walk is csgpu_solve_many_clauses's -- root row checks and the root node, the counters, max_nodes compared before a
 * child is tried, a child entered at once and its parent pushed only if it has children left, ANY / ALL / MIN / MAX, the
 * private incumbent and its bound on dom[obj] before every child's fixpoint, d_best and d_solutions -- with two changes.
 *   Branching.  The branching variable is the open variable with the smallest csgpu_branch_key(order, 0, value, 0,
 *               index): order 0 none, 1 smallest domain, 2 largest domain, 3 smallest value (the lowest lo), 4 largest
 *               value (the highest hi), ties to the lowest index, over all variables including "<obj>".  The key's
 *               domain size saturates as csgpu_branch_key's does: an interval with a bound at INT32_MIN or INT32_MAX
 *               (the reference's infinities), or of 2^31 values or more, has the largest size there is, 2^31 - 1, so
 *               among such intervals orders 1 and 2 choose by index alone.  (csgpu_solve_many_clauses compares hi - lo
 *               in full; the two walks are the same tree for order 1 wherever no open interval saturates and nothing
 *               halves.)
 *   Children.   A node whose branching variable has more than split_width values -- hi - lo + 1, in 64 bits -- has two
 *               children: [lo, mid] first, then [mid + 1, hi], mid = (lo + hi) >> 1, a floor taken in 64 bits.  Any
 *               other node has its values in ascending order.  Whether a node halves, and its mid, are fixed by the
 *               node's row as it was entered, before any incumbent bound: a frame popped later makes the same children.
 *               A half is "narrow the variable to that half, then the fixpoint": a node in `nodes`, and a cut if the
 *               fixpoint fails or the incumbent's bound empties dom[obj].  The second half is its node's last child.
 *   d_halvings  NULL, or [count] int64: the parents of the instance that were split in two, each counted once, when its
 *               first half is tried.  0 for a row that is not searched.
 * Prefer-failing is not part of this walk: which variable a failed fixpoint blames depends on kernel 6's revision order.
 * Frames.  A pushed halving parent values no variable, so a wave's stack can be deeper than n_vars.
 * csgpu_many_clauses_ordered_frames(m, split_width) is the frames per wave of a call, from the model's root domains alone
 * and without a HIP call: n_vars + the sum over the variables of h(v), h(v) the smallest h for which the root width,
 * halved h times with ceiling, is at most split_width (0 means 256) -- rows lie inside the root domains and intervals only
 * shrink along a path.  0 for a model that does not qualify, or a negative split_width.  The call launches
 * min(count, resident waves) waves, fewer where their frames would pass 1 GiB, as csgpu_solve_many_clauses does; the
 * kernel compares the depth with that count before it writes all the same (CSGPU_MANY_LIMIT).
 * Errors before any HIP call: csgpu_solve_many_clauses's in its order (options is this entry's struct), then an order
 * outside 0 .. 4, a negative split_width or a non-zero `reserved` -> CSGPU_E_ARG.  count == 0 -> CSGPU_OK, nothing is
 * launched.
 * Not on this walk: up to k solutions, the solution stream, restarts, prefer-failing, and the kernel-7 walks of
 * csgpu_solve_many, which keep their one rule.  Checkpoints and resume are the section after this one, start incumbents
 * and the spread over idle waves the one after that. */
typedef struct csgpu_many_order_options {
  int32_t objective;   /* 0 ANY, 1 ALL, 2 MIN, 3 MAX */
  int32_t order;       /* 0..4, csgpu_search_set_strategy's numbers */
  int32_t split_width; /* >= 1; 0 means 256, the engine's */
  int32_t reserved;    /* 0 */
  int64_t max_nodes;
} csgpu_many_order_options;
int csgpu_solve_many_clauses_ordered(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                     const csgpu_many_order_options *options, csgpu_many_result *d_results,
                                     int32_t *d_solutions /* NULL or [count][n_vars] */, int32_t *d_best /* NULL or [count] */,
                                     int64_t *d_halvings /* NULL or [count] */, void *stream);
int64_t csgpu_many_clauses_ordered_frames(const csgpu_model *m, int32_t split_width);

/* ---- ordered clause checkpoints: csgpu_solve_many_clauses_ordered in slices ----
 * A launch of csgpu_solve_many_clauses_ordered lasts as long as its deepest instance.  These calls are to it what
 * csgpu_solve_many_clauses_checkpointed / _resume are to csgpu_solve_many_clauses: a small budget for everybody, then more
 * for the few that need it, or the rest handed to one csgpu_search.
 *
 * The walk is csgpu_solve_many_clauses_ordered's, the contract csgpu_solve_many_clauses_checkpointed / _resume's: max_nodes
 * is the budget of THIS call; instances with d_slots[i] < 0 are untouched by a resume (record, row, best, halving count);
 * an instance ends DONE with d_slots[i] = -1, or LIMIT with its header and {variable, next} back in the same slot; once
 * the pool is exhausted an instance ends LIMIT with slot -1, as without checkpoints; one call is in flight per model, and
 * calls may be queued on one stream.  A resume takes no roots and needs no workspace.
 * Guarantee: a walk in slices gives, field for field and row for row, d_halvings included, the one
 * csgpu_solve_many_clauses_ordered call with the summed budget.
 *
 * The pool.  A pushed halving parent values no variable, so a stack is deeper than n_vars and a slot of
 * csgpu_many_clause_checkpoints_create does not hold it.  With F = csgpu_many_clauses_ordered_frames(m, split_width):
 *   slot = F + 1 frames of n_vars + 1 entries of 8 bytes, bounds absolute
 *   frame 0           the header: entry 0 = {depth, magic}, entry 1 = {best, have_best | code << 1}, code = objective |
 *                     order << 3; the magic is not that of a csgpu_many_clause_checkpoints_create slot
 *   frame 1 + d       pushed frame d < depth: the row, then {variable, next}: the next value, or mid + 1 of a halving node
 *   frame 1 + depth   the current node as it was entered and {variable, next}: next == lo of a halving node means that
 *                     neither half was tried, next == mid + 1 that the second half is next
 * F + 1 frames because F - 1 parents at most are pushed under the current node, and frame 0 is the header.  Whether a
 * frame's node halves, and its mid, are read back from the frame's row, so a walk stopped between the two halves counts
 * the parent once.  csgpu_many_clause_ordered_checkpoint_bytes(m, split_width) is the bytes of a slot, (F + 1) * (n_vars +
 * 1) * 8 in 64 bits, without a HIP call (0 means 256); 0 for NULL, a model that does not qualify or a negative
 * split_width.  csgpu_many_clause_ordered_checkpoints_create makes a pool for ONE split_width (a negative one ->
 * CSGPU_E_ARG; everything else as csgpu_many_clause_checkpoints_create); csgpu_many_checkpoints_reset / _free serve it.
 * A resume under another objective or another order would walk another tree: the slot's code differs and the instance ends
 * CSGPU_MANY_BAD_SLOT, as for a slot number outside the pool or a slot that holds no checkpoint, with only its status
 * word written.  The halving count of a resumed instance goes on from d_halvings[i], as the other counters go on from the
 * record: d_halvings is required.
 *
 * Errors before any HIP call, in this order: csgpu_solve_many_clauses_checkpointed's null arguments, count and max_nodes;
 * csgpu_solve_many_clauses's objective, model and count checks; an order outside 0 .. 4, a negative split_width, a
 * non-zero `reserved` -> CSGPU_E_ARG; d_halvings NULL -> CSGPU_E_ARG; ck or d_slots NULL, a pool of another model, a pool
 * of csgpu_many_checkpoints_create or csgpu_many_clause_checkpoints_create -> CSGPU_E_ARG; a pool made for another
 * split_width (both normalised, 0 to 256) -> CSGPU_E_ARG.  count == 0 -> CSGPU_OK, nothing is launched.
 * csgpu_many_clause_checkpoint_states takes a pool of this kind as well and returns up to F states by the one rule: a frame
 * {row, variable, next} is the row with the variable narrowed to [next, hi] -- for a pushed halving parent exactly its
 * second half, for a current node before its first half the whole node.  Every other entry that takes a clause pool
 * refuses this kind with CSGPU_E_ARG: csgpu_solve_many_clauses_checkpointed / _resume, the up-to-k calls, _from /
 * _from_resume, the stream, and csgpu_many_clause_checkpoint_children / _fanout and their _obj forms.  The spread over
 * idle waves has entries of its own for this kind (the next section): a fan-out of halves has to account for `halvings`.
 * Not built on the ordered walk: up to k solutions, the solution stream, restarts and prefer-failing. */
size_t csgpu_many_clause_ordered_checkpoint_bytes(const csgpu_model *m, int32_t split_width);
int csgpu_many_clause_ordered_checkpoints_create(const csgpu_model *m, int64_t capacity, int32_t split_width,
                                                 csgpu_many_checkpoints **out);
int csgpu_solve_many_clauses_ordered_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                                  const csgpu_many_order_options *options, csgpu_many_result *d_results,
                                                  int32_t *d_solutions /* NULL or [count][n_vars] */,
                                                  int32_t *d_best /* NULL or [count] */, int64_t *d_halvings /* [count] */,
                                                  csgpu_many_checkpoints *ck, int32_t *d_slots /* [count] */, void *stream);
int csgpu_solve_many_clauses_ordered_resume(const csgpu_model *m, int64_t count, const csgpu_many_order_options *options,
                                            csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                            int64_t *d_halvings, csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);

/* ---- the ordered walk: start incumbents, and stopped walks spread over the waves of the next call ----
 * What "start incumbents" and the two spreads above are to csgpu_solve_many_clauses, for csgpu_solve_many_clauses_ordered:
 * a launch lasts as long as its deepest instance, so the open children of the stopped instances -- halves included -- are
 * counted and fanned out on the device, walked by the other waves, and folded back into their owners.
 *
 * Start incumbents (kernel cs_walk_order_from).  csgpu_solve_many_clauses_ordered_from / _from_resume are
 * csgpu_solve_many_clauses_from / _from_resume on the ordered walk: `starting`, `own solutions` and `resuming` above hold
 * word for word, with csgpu_solve_many_clauses_ordered[_checkpointed] for csgpu_solve_many_clauses[_checkpointed] -- with
 * have == 0 everywhere the call is that one, field for field and row for row, d_halvings included -- and the slots are
 * those of a csgpu_many_clause_ordered_checkpoints_create pool, code = objective | order << 3.  MIN / MAX only.  A
 * checkpoint of either ordered MIN / MAX call may be resumed by either ordered resume.
 *   csgpu_solve_many_clauses_ordered_from         d_start [count] is required; ck == NULL and d_slots == NULL: the plain call
 *                                                 (d_halvings NULL or [count]); both given: the checkpointed call (d_halvings
 *                                                 [count] is required, as for every ordered call with a pool)
 *   csgpu_solve_many_clauses_ordered_from_resume  as csgpu_solve_many_clauses_ordered_resume
 * Errors before any HIP call, in this order: those of csgpu_solve_many_clauses, in its order and with its codes; an order
 * outside 0 .. 4, a negative split_width, a non-zero `reserved` -> CSGPU_E_ARG; a null d_start, an objective ANY / ALL,
 * exactly one of ck / d_slots null (the resume: either) -> CSGPU_E_ARG; with a pool: d_halvings NULL, a pool of another
 * model, a pool of csgpu_many_checkpoints_create or csgpu_many_clause_checkpoints_create, a pool made for another
 * split_width -> CSGPU_E_ARG; then count == 0 -> CSGPU_OK.
 *
 * The children of a stopped walk.  A slot's frame {row f, variable bv, next}, with lo, hi = f[bv] and mid = (lo + hi) >> 1
 * taken in 64 bits, has the children the walk itself would try next:
 *   enumerating (hi - lo + 1 <= split_width), next in [lo, hi]   the rows bv = [v, v] for v = next .. hi
 *   halving, next == mid + 1 (the second half is left)           one child, bv = [mid + 1, hi]
 *   halving, next == lo (neither half tried)                     two children, bv = [lo, mid], then bv = [mid + 1, hi]
 * The third case is possible for the current node only (frame 1 + depth).  There the walk has not yet counted the parent in
 * its halving count (it does when the first half is tried): the instance owes one halving that no record holds, and
 * d_unsplit[i] = 1 for such a slot, else 0.  Walk order: the current node's children first, then those of the frame below
 * it, down to the oldest.  The split width is the pool's.
 *   csgpu_many_clause_ordered_checkpoint_children  d_children[i] = the children of slot d_slots[i], in 64 bits: 0 for
 *                                                  d_slots[i] < 0, -1 for a refused slot; d_unsplit [count] int32
 *   csgpu_many_clause_ordered_checkpoint_fanout    d_rows[d_offsets[i] ..] = the children of instance i as root rows in walk
 *                                                  order, d_owner[row] = i (d_owner may be NULL); d_offsets [count + 1].
 *                                                  The slot is counted again first: nothing of instance i is written unless
 *                                                  d_offsets[i + 1] - d_offsets[i] is exactly its count and its rows lie
 *                                                  inside [0, total)
 * Everything is compared before what depends on it is read.  A slot is refused -- count -1, nothing written, never a
 * partial count -- for a slot number at or above the capacity, another magic, a depth outside [0, F), a code that is not
 * exactly objective | order << 3 of the call, a frame whose bv is outside [0, n_vars), a frame whose bounds of bv are
 * empty or outside the root domain, an enumerating frame whose next lies outside [lo, hi], a halving frame whose next is
 * neither mid + 1 nor, for the current node only, lo.
 * objective is ALL, MIN or MAX.  Under ALL d_owner_start and d_start must be NULL and the rows are walked by
 * csgpu_solve_many_clauses_ordered_checkpointed; under MIN / MAX d_start [total] is required, d_start[row] is the better --
 * strictly, by csgpu_objective_better's order -- of the slot's header incumbent and d_owner_start[i] (NULL, or [count];
 * have == 0: none), as csgpu_many_clause_checkpoint_fanout_obj writes it, and the rows are walked by
 * csgpu_solve_many_clauses_ordered_from.
 * Errors before any HIP call, in this order: a null ck / d_slots / d_children / d_unsplit (the fan-out: ck / d_slots /
 * d_offsets / d_rows), count < 0, (the fan-out) total < 0 -> CSGPU_E_ARG; an objective other than ALL / MIN / MAX (ANY
 * among them), an order outside 0 .. 4 -> CSGPU_E_ARG; a pool of csgpu_many_checkpoints_create or
 * csgpu_many_clause_checkpoints_create -> CSGPU_E_ARG; count > 2^31 - 1 -> CSGPU_E_LIMIT; (the fan-out) under ALL a
 * d_owner_start or d_start that is not NULL, under MIN / MAX a null d_start -> CSGPU_E_ARG; then count == 0 (the fan-out:
 * or total == 0) -> CSGPU_OK.
 *
 * The fold.  A child walked as a root row of its own is what the walk makes of it: the row narrowed, the fixpoint, the
 * branching variable chosen anew.  The records fold with the unchanged csgpu_many_fold and the best values with the
 * unchanged csgpu_many_fold_best.  An owner's halving count is its own, plus d_unsplit of each of its fanned slots, plus
 * the counts of its sub-instances:
 *   csgpu_many_fold_halvings   for every t < total with d_owner[t] >= 0: one relaxed agent-scope 64-bit add of
 *                              d_sub_halvings[t] to d_halvings[d_owner[t]].  Once per batch.  Errors: a null pointer,
 *                              total < 0 -> CSGPU_E_ARG; total > 2^39 - 256 -> CSGPU_E_LIMIT; then total == 0 -> CSGPU_OK
 * Under ALL the fold is exact: an owner whose sub-instances all ended DONE has the record of the one
 * csgpu_solve_many_clauses_ordered call, field for field, and its halving count.  Under MIN / MAX it is exact for the
 * optimum and its proof (status DONE and best are the one call's); the walk that was made is larger than the one call's. */
int csgpu_solve_many_clauses_ordered_from(const csgpu_model *m, const csgpu_val *d_roots, const csgpu_many_start *d_start,
                                          int64_t count, const csgpu_many_order_options *options, csgpu_many_result *d_results,
                                          int32_t *d_solutions, int32_t *d_best, int64_t *d_halvings, csgpu_many_checkpoints *ck,
                                          int32_t *d_slots, void *stream);
int csgpu_solve_many_clauses_ordered_from_resume(const csgpu_model *m, int64_t count, const csgpu_many_order_options *options,
                                                 csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                                 int64_t *d_halvings, csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);
int csgpu_many_clause_ordered_checkpoint_children(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                  int objective, int order, int64_t *d_children, int32_t *d_unsplit, void *stream);
int csgpu_many_clause_ordered_checkpoint_fanout(const csgpu_many_checkpoints *ck, const int32_t *d_slots, int64_t count,
                                                int objective, int order, const csgpu_many_start *d_owner_start,
                                                const int64_t *d_offsets, csgpu_val *d_rows, int32_t *d_owner,
                                                csgpu_many_start *d_start, int64_t total, void *stream);
int csgpu_many_fold_halvings(const int64_t *d_sub_halvings, const int32_t *d_owner, int64_t total, int64_t *d_halvings,
                             void *stream);

/* ---- clause models past 512 clauses: csgpu_solve_many_clauses with the clause records in LDS ----
 * csgpu_solve_many_clauses and everything built on it walk on kernel 6's fixpoint, which keeps every clause record in
 * registers: 512 clauses at most, CSGPU_E_LIMIT above.  That limit is the register file's, not the walk's.  These calls
 * are an entry of their own, opt-in, for which a workgroup stages the records once in LDS -- 16 bytes per clause and 32
 * more per two-literal disjunction, one copy for the workgroup's four waves -- and every wave reads its clause of a slot
 * from there (cs_walk_wide, cs_walk_wide_resume).  The existing entries keep refusing what they refused.
 * THE WALK IS csgpu_solve_many_clauses's, by reference: the node, the branching variable (smallest hi - lo, ties to the
 * lowest index), the ascending values, the child and its rounds, the private incumbent under MIN / MAX, the stored row,
 * d_best, the counters (nodes, cuts, solutions, props, root_props), the statuses (DONE, LIMIT, BAD_ROOT; BAD_SLOT from a
 * resume), max_nodes compared before a child is tried, a root row outside the root domains, the objective checks, the
 * concurrency rule and count == 0 are all defined there and in "clause checkpoints" above.  Two things differ:
 *   where the records live   in LDS, not in registers.  The order is the same (the records sorted by kind, clause
 *                            lane + 64 q in slot q, the slots in ascending order), so on a model both entries take every
 *                            field of every record is the same, props and root_props included
 *   which models qualify     every finalized model with at least one clause whose staged block and the LDS slices of a
 *                            workgroup's four waves fit the 160 KiB of a CU: 16 (clauses + 2 disjunctions) +
 *                            4 ((8 n_vars + 16) rounded up to 16) bytes.  Models of at most 512 clauses qualify too.
 *                            csgpu_model_qualifies_many_clauses_wide says so: after finalize what was planned, after
 *                            csgpu_model_build_tables alone the same rule on the host tables (no HIP call)
 * A model that does not fit -> CSGPU_E_LIMIT, and the message names the bytes it needs and the 160 KiB.
 * Checkpoints: csgpu_solve_many_clauses_wide_checkpointed / _wide_resume are csgpu_solve_many_clauses_checkpointed /
 * _resume, slot layout, header and codes included; a slot is csgpu_many_clause_wide_checkpoint_bytes(m) =
 * (n_vars + 1)^2 x 8 bytes (0 if the model does not qualify, and for NULL; no HIP call).  The pool is of a kind of its
 * own, made by csgpu_many_clause_wide_checkpoints_create: every other entry that takes a pool -- the resumes, _children,
 * _fanout and _states of all three older kinds -- refuses it with CSGPU_E_ARG, as the wide entries refuse a pool of
 * another kind; csgpu_many_checkpoints_reset and _free serve it as any pool.  A resume under another objective than the
 * checkpoint's is CSGPU_MANY_BAD_SLOT per instance, as on the plain walk.
 * Errors before any HIP call, in csgpu_solve_many_clauses's order and with its codes, the model's own check in the place
 * of "at most 512 clauses".
 * Not here (each is out of scope for the wide walk and stays with the entries above, at most 512 clauses): up to k
 * solutions, the stream and restarts; the variable orders and halving; start incumbents; the spread over idle waves and
 * csgpu_many_clause_checkpoint_states with the Search finish; the sliced drivers.  Kernel 6 itself (csgpu_propagate_batch
 * with kernel 6, the engine) keeps its 512, and a model whose block does not fit LDS is not read through L2 instead. */
int csgpu_model_qualifies_many_clauses_wide(const csgpu_model *m);
int csgpu_solve_many_clauses_wide(const csgpu_model *m, const csgpu_val *d_roots, int64_t count, const csgpu_many_options *options,
                                  csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best, void *stream);
size_t csgpu_many_clause_wide_checkpoint_bytes(const csgpu_model *m);
int csgpu_many_clause_wide_checkpoints_create(const csgpu_model *m, int64_t capacity, csgpu_many_checkpoints **out);
int csgpu_solve_many_clauses_wide_checkpointed(const csgpu_model *m, const csgpu_val *d_roots, int64_t count,
                                               const csgpu_many_options *options, csgpu_many_result *d_results,
                                               int32_t *d_solutions, int32_t *d_best, csgpu_many_checkpoints *ck,
                                               int32_t *d_slots, void *stream);
int csgpu_solve_many_clauses_wide_resume(const csgpu_model *m, int64_t count, const csgpu_many_options *options,
                                         csgpu_many_result *d_results, int32_t *d_solutions, int32_t *d_best,
                                         csgpu_many_checkpoints *ck, int32_t *d_slots, void *stream);

/* Three-valued evaluation of the root wide-and for a batch of states:
 * d_truth[i] = 1 (all clauses true), 0 (some clause false), 2 (undecided). */
int csgpu_eval_batch(const csgpu_model *m, const csgpu_val *d_states, int32_t *d_truth, int64_t batch,
                     void *stream);

/* Interval value of every clause (top-level constraint) for ONE state: the eval_<op>
 * entry points of the reference (eval.c:27-255) applied to each clause root.
 * d_vals: device, [n_clauses] csgpu_val. */
int csgpu_eval_clauses(const csgpu_model *m, const csgpu_val *d_state, csgpu_val *d_vals, void *stream);

/* ---- device-resident tree search (the batched analogue of solve(), csolve.c:398-476) ----
 *
 * A LIFO pool of open states lives in HBM.  One iteration pops the newest states, branches each
 * on its first open variable (every value of its interval becomes a child, as step_val
 * enumerates them, csolve.c:331-338), propagates all children in one csgpu_propagate_batch_obj
 * launch, counts the inconsistent ones as cuts, checks complete assignments with the root
 * evaluation (update_solution, csolve.c:222-244) and pushes the open survivors back.
 * The search tree is the reference's (same children, same propagation per child); the ORDER in
 * which it is walked is not, so CALLS/CUTS are engine-specific while the set of solutions and
 * the optimum are not.  Subtree sharding across GPUs moves whole states between the pools of
 * different ranks (csgpu_search_take / _put) and exchanges the incumbent (_set_best).
 * When the states carry one forbidden-set word per variable, a child whose value the parent's own
 * set already forbids (a valued neighbour rules it out, so its propagation can only fail) is counted
 * in `nodes` and `cuts` without being launched; CSGPU_SEARCH_HOLES=0 launches those too (same
 * counts, same solutions). */
typedef struct csgpu_search csgpu_search;

typedef struct csgpu_search_stats {
  uint64_t nodes;      /* children = CALLS */
  uint64_t cuts;       /* inconsistent children = CUTS */
  uint64_t props;      /* narrowing events = PROPS */
  uint64_t revisions;  /* clause revisions */
  uint64_t solutions;  /* accepted solutions (root evaluates to true) */
  uint64_t iterations; /* batched expand+propagate rounds */
  uint64_t restarts;   /* ANY only: Luby restarts (check_restart, csolve.c:264-276) */
  int64_t pool;        /* open states now in the pool */
  int64_t pool_peak;
  int32_t best;        /* incumbent (MIN/MAX), INT32_MAX / INT32_MIN if none yet */
  int32_t done;        /* 1: pool empty, or objective ANY and a solution was found */
} csgpu_search_stats;

/* pool_capacity: states the pool can hold; max_children: children propagated per iteration */
int csgpu_search_create(const csgpu_model *m, int64_t pool_capacity, int64_t max_children, csgpu_search **out);
void csgpu_search_free(csgpu_search *s);
/* forget everything (pool, statistics, incumbent, stored solutions, restart seeds) but keep the
 * buffers: the engine can run another search on the same model */
int csgpu_search_reset(csgpu_search *s);
/* append `count` states ([count][n_vars], device memory) to the pool */
int csgpu_search_put(csgpu_search *s, const csgpu_val *d_states, int64_t count);
/* the same from host memory (e.g. the root domains of csgpu_model_get_domains) */
int csgpu_search_put_host(csgpu_search *s, const csgpu_val *states, int64_t count);
/* remove up to `max` of the OLDEST states (the largest subtrees) into d_states; *count = how many */
int csgpu_search_take(csgpu_search *s, csgpu_val *d_states, int64_t max, int64_t *count);
/* the same into host memory (states: [max][n_vars]), the twin of csgpu_search_put_host */
int csgpu_search_take_host(csgpu_search *s, csgpu_val *states, int64_t max, int64_t *count);
/* cap on the open states expanded per iteration (default: as many as max_children allows for
 * ALL; 64 for ANY/MIN/MAX, which makes the walk depth-first enough to reach a first solution or a
 * good incumbent early with a small pool; MIN/MAX go up to 256 while the pool holds a backlog of
 * more than 16 x as many open states).  A value set here is taken literally. */
int csgpu_search_set_parents(csgpu_search *s, int64_t parents_per_iteration);
/* ANY only: restart from the seeded states after luby(i) x `iterations` iterations without a
 * solution (the reference restarts after luby(i) x restart_frequency failures, csolve.c:76-83,
 * 264-276, default 100); every restart tries the values in a different pseudo-random rotation.
 * Default 64; 0 disables restarts. */
int csgpu_search_set_restart(csgpu_search *s, int64_t iterations);
/* The reference's strategy options (src/main.c:51-130, src/strategy.c:79-121), to be set before the first state is put.
 * order: which open variable is branched on first -- 0 none, 1 smallest domain (default), 2 largest domain, 3 smallest
 * value, 4 largest value (-o); prefer_failing != 0: among equals the variable with the highest failure count (-f):
 * the branching variable's count goes down when an assignment holds and up when it fails, the variable whose domain
 * emptied goes up (csolve.c:455-465, propagate.c:33-41; the reference's further bumps along its recursion stack follow
 * its depth-first order and have no counterpart in a batch).  Ties: lowest index (the reference: heap order).
 * Anything but the default (1, 0) takes the separate-kernel path on interval rows; with failure counts the tree of
 * a search depends on the order in which batches finish. */
int csgpu_search_set_strategy(csgpu_search *s, int order, int prefer_failing);
/* MIN / MAX: a better solution restarts the search from the states it was seeded with, under the new bound
 * (update_solution + is_solution_restartable, csolve.c:216-219, 418-425).  Off by default. */
int csgpu_search_set_restart_on_improvement(csgpu_search *s, int on);
/* host time csgpu_search_put / put_host have taken since the last reset (device copy + rebuilding the forbidden
 * sets of the arriving states, which travel between ranks without them) and the states they brought */
int csgpu_search_put_cost(const csgpu_search *s, double *seconds, int64_t *states);
/* ---- helpers of the search driver -----------------------------------------------------------------------------
 * Host functions, no device needed.  The same code (csolve_amd/csrc/cs_arith.h) runs inside the kernels
 * (incumbent bound), the engine (restart schedule) and the drop-in (order of sibling values); exported so the
 * reference's unit vectors (test/test_objective.c, test/test_csolve.c:305-337,628-657) can be run against it.
 * `objective`: as returned by csgpu_model_objective (0 ANY 1 ALL 2 MIN 3 MAX). */
/* objective_better (objective.c:62-78): can objective value `value` still beat the incumbent `best`? */
int csgpu_objective_better(int objective, csgpu_val value, int32_t best);
/* objective_update_val (objective.c:101-126): `value` under the incumbent bound (MIN: hi <= best - 1) */
csgpu_val csgpu_objective_bound(int objective, csgpu_val value, int32_t best);
/* objective_update_best (objective.c:81-98): the incumbent after a solution with objective value `value` */
int32_t csgpu_objective_best(int objective, csgpu_val value, int32_t best);
/* fail_threshold_next (csolve.c:76-83): the next element of the Luby sequence 1 1 2 1 1 2 4 ... */
void csgpu_luby_next(uint64_t *threshold, uint64_t *counter);
/* step_check / step_val (csolve.c:323-338): is iteration `iter` over `bounds` valid, and the value it tries */
int csgpu_step_check(csgpu_val bounds, uint32_t iter);
int32_t csgpu_step_val(csgpu_val bounds, uint32_t iter, uint32_t seed);
/* strategy_var_cmp (strategy.c:79-121) as a key: the engine branches on the open variable with the SMALLEST key (what
 * the reference's heap has on top); order 0 none / 1 smallest domain / 2 largest domain / 3 smallest value / 4 largest
 * value, then (prefer_failing) the higher failure count, then the lower index.  sign(strategy_var_cmp(a, b)) =
 * sign(key(b) - key(a)) with the index bits masked (test/test_strategy.c VarCmp.*). */
uint64_t csgpu_branch_key(int order, int prefer_failing, csgpu_val value, int64_t prio, int32_t index);

/* merge an incumbent found elsewhere (objective_best of the shared page, objective.c:89-93) */
int csgpu_search_set_best(csgpu_search *s, int32_t best);
/* MIN / MAX engines of the same model on one device: from now on `s` keeps its incumbent in `with`'s word of
 * device memory (the analogue of the reference's shared page, csolve.c:86-97): what one engine accepts bounds
 * the very next fixpoints of the other.  If `with` borrows itself, `s` borrows from the same owner; an engine
 * that lends cannot borrow (CSGPU_E_STATE).  Lifetime: csgpu_search_free of a lender is deferred by the library
 * until its last borrower has been freed (the handle must not be used after the call all the same).
 * csgpu_search_reset of either resets the word.  Needs the device-driven iterations (CSGPU_E_STATE otherwise),
 * and while shared csgpu_search_set_parents refuses a setting that would leave them (CSGPU_E_STATE).
 * csgpu_search_best_solution answers 1 only on the engine whose stored row attains the current incumbent
 * (after csgpu_search_run / csgpu_search_set_best have brought its statistics up to date); the others answer 0.
 * With several engines accepting concurrently, node counts of a MIN / MAX run depend on timing; the optimum
 * does not.  A no-op for ANY / ALL. */
int csgpu_search_share_incumbent(csgpu_search *s, csgpu_search *with);
/* run up to max_iterations iterations (stops early when done).  ANY/MIN/MAX iterations are enqueued
 * sixteen at a time as one hipGraph with the bookkeeping between them on the device (pool top, child
 * counts, incumbent, stop conditions); the host reads the totals once per sixteen.  Environment, read
 * at csgpu_search_create: CSGPU_SEARCH_BURST=0 drives every iteration from the host,
 * CSGPU_SEARCH_GRAPH=0 enqueues the launches one by one instead of as a graph. */
int csgpu_search_run(csgpu_search *s, int64_t max_iterations, csgpu_search_stats *stats);
/* copy up to `max` stored solutions ([k][n_vars] values, host memory); returns k */
int64_t csgpu_search_solutions(const csgpu_search *s, int32_t *values, int64_t max);

/* ---- the solution stream: every solution to the caller, not only the first 1,024 of the store above ----
 * Off by default; nothing changes while it is off.  csgpu_search_set_solution_stream turns it on with room for `rows`
 * rows of n_vars int32 values in device memory; set before the first state is put (CSGPU_E_STATE otherwise, and on
 * an engine that shares an incumbent in either direction -- csgpu_search_share_incumbent then refuses too);
 * rows < the widest root interval (the children of one parent at most) is CSGPU_E_ARG.
 * What the kernels append, per objective:
 *   ALL       every accepted solution, once: over a whole search the rows drained = stats.solutions;
 *   ANY       the one accepted solution (the row csgpu_search_solutions gives);
 *   MIN / MAX per iteration, the accepted solution that improved the incumbent, if one did (what the reference prints,
 *             update_solution, csolve.c:222-244): objective values strictly improving, the last row attains
 *             stats.best and equals csgpu_search_best_solution's.
 * With the stream on, csgpu_search_run returns early (CSGPU_OK, done == 0) when the stream cannot take the worst case
 * of the next iteration (ALL: room for every child of every parent it expands -- the iteration is sized so) or burst
 * (one row per iteration); a row is never dropped nor written twice, and a kernel that still finds no room makes the
 * call return CSGPU_E_LIMIT.  After that error the engine must be reset: until then csgpu_search_run, the drains and
 * csgpu_search_pending_solutions answer CSGPU_E_STATE (what the kernels had appended is not trusted).
 * The caller's loop: while (!st.done) { csgpu_search_run(s, N, &st); drain(...); }.
 * The stream is a ring: a drain copies the rows it returns and moves nothing else, so draining in small batches costs
 * what the batches hold.  csgpu_search_reset empties the stream and keeps it on. */
int csgpu_search_set_solution_stream(csgpu_search *s, int64_t rows);
/* move up to `max` waiting rows, oldest first, into `values` ([k][n_vars], host memory); *count = k (max = 0: none,
 * the stream is left as it is).  Rows left over stay for the next call.  What the engine still holds back (the accept
 * of its last iteration) is flushed first. */
int csgpu_search_drain_solutions(csgpu_search *s, int32_t *values, int64_t max, int64_t *count);
/* the same into device memory, ordered on `stream` (a hipStream_t, NULL = the null stream); returns when it is done */
int csgpu_search_drain_solutions_device(csgpu_search *s, int32_t *d_values, int64_t max, int64_t *count, void *stream);
/* rows waiting in the stream and rows it has room for (after csgpu_search_run or a drain: exact) */
int csgpu_search_pending_solutions(const csgpu_search *s, int64_t *rows, int64_t *room);

/* MIN/MAX: the values ([n_vars], host memory) of a solution that attains the incumbent
 * (csgpu_search_stats.best); returns 1 if there is one, 0 if no solution was found yet */
int csgpu_search_best_solution(const csgpu_search *s, int32_t *values);

/* ---- the sharded search of one node: one engine per rank (process), coordinated in host C (cs_shard.c) ----
 * The reference forks a worker that takes half of the branching interval whenever a slot is free, and its workers
 * share one page: the incumbent, the solutions found, the timeout flag (csolve.c:86-152, 190-244).  Here the ranks
 * exist up front, rank 0 expands the root and deals its frontier out, and the ranks exchange open states (the OLDEST of
 * a pool: whole subtrees), the incumbent and their status through a REGION of shared memory that every rank of the
 * node maps.  The protocol is that of ShardedSearch (csolve_amd/parallel.py); INTEGRATION.md describes it.
 *
 * csgpu_plan_transfers: the rebalancing plan from the ranks' pool sizes, the same on every rank (parallel.py
 * plan_transfers): pair the richest rank with the poorest while the poorest holds fewer than `low_water` states and
 * give half the difference, at most `max_give` (>= 1).  plan: room for world / 2 rows of {src, dst, count};
 * *count = rows.  1 <= world <= 1024. */
int csgpu_plan_transfers(const int64_t *pools, int world, int64_t low_water, int64_t max_give, int64_t *plan,
                         int *count);
/* The region: a process-shared lock and barrier (waits sleep), per rank the status words (waiting at exchange,
 * incumbent, found, pool, timed out), the exchange table and final counters, and an inbox of `inbox_rows` states
 * ([inbox_rows][n_vars] csgpu_val); the solutions reported on the node.  Host-only, no device: the launcher sizes it,
 * places it in memory every rank maps (MAP_SHARED), and initialises it once before any rank starts.  One region serves
 * one search.  1 <= world <= 8 (one rank per GPU of a node), n_vars >= 1, inbox_rows >= 1; CSGPU_E_ARG otherwise, and
 * when `bytes` is short of the size. */
#define CSGPU_SHARD_MAX_WORLD 8
int csgpu_shard_region_size(int world, int n_vars, int64_t inbox_rows, size_t *bytes);
int csgpu_shard_region_init(void *region, size_t bytes, int world, int n_vars, int64_t inbox_rows);
/* every rank of the region waits here until all have arrived */
int csgpu_shard_barrier(void *region);
/* the number of variables of a problem text, for a launcher sizing the region: the host front end alone (no device, no
 * HIP call; csgpu_model_free is a device call).  CSGPU_E_PARSE with the front end's message. */
int csgpu_text_num_vars(const char *text, int weights_on, int *n_vars);

/* rows: [count][n_vars] values; best: the objective value of the row (MIN / MAX), 0 for ANY / ALL.  Called with the
 * region's lock held, so what one rank writes never interleaves with another's output. */
typedef void (*csgpu_shard_solution_fn)(void *user, int rank, const int32_t *rows, int64_t count, int32_t best);

typedef struct csgpu_shard_options {
  int64_t slice_iterations;     /* iterations between exchanges (64) */
  int64_t poll_iterations;      /* a slice runs in bursts of this many; the region is looked at between them (4) */
  int64_t seed_states_per_rank; /* rank 0 expands the root until its pool holds this many x world (64) */
  int64_t low_water;            /* a rank with fewer open states is given some at an exchange (64) */
  double time_limit;            /* seconds, 0 = none: every rank stops at the same exchange (-t) */
  csgpu_shard_solution_fn on_solution; /* nullable */
  void *user;
} csgpu_shard_options;
void csgpu_shard_default_options(csgpu_shard_options *options);

/* One rank's whole search on engine `s` (fresh: nothing put, nothing run; a solution stream, if on, is drained here).
 * Every rank of the region calls it with its own engine of the same model and the same options; rank 0 passes the
 * root state ([n_vars], host memory), the others NULL.  Solutions go to options->on_solution as they are found:
 *   ALL       every row, as the engine's solution stream gives it (the stream must be on when there is a callback);
 *   ANY       the node's first row only;
 *   MIN / MAX one row at the end: the row attaining the node's optimum, of the lowest rank that holds one.
 * local: this rank's engine statistics (rank 0's include expanding the root).  totals: the counters summed over the
 * ranks, best = min / max over them, pool = what was left open (non-zero after a time limit), done = nothing left
 * open or ANY solved; solutions = ALL: the rows (the sum over ranks), ANY: 1 if one was found, MIN / MAX: the sum of
 * the ranks' accepted solutions.  With world > 1, an engine whose restarts are on (csgpu_search_set_restart > 0 for
 * ANY, which is the default, or csgpu_search_set_restart_on_improvement) is refused with CSGPU_E_STATE before the
 * rank touches the region: a restart re-puts the states put before the first iteration and would drop what the rank
 * was given later.  world == 1 runs the same search as csgpu_search_run to completion.  A rank whose call fails
 * leaves the others waiting at the next barrier: the launcher ends them (the command line's -j does). */
int csgpu_shard_run(csgpu_search *s, void *region, int rank, const csgpu_val *root, const csgpu_shard_options *options,
                    csgpu_search_stats *local, csgpu_search_stats *totals);

/* `count` values of variable `var` on ONE parent state, host buffers: node i assigns values[i].  results and
 * states_out ([count][n_vars]; rows of inconsistent nodes unspecified) are host memory.  What the reference
 * driver asks for one value at a time (step_val, csolve.c:331-338 -> check_assignment, csolve.c:247-261), in one
 * launch; the drop-in shim serves the driver's following calls from it.  Synchronous. */
int csgpu_propagate_values(const csgpu_model *m, const csgpu_val *state, int32_t var, const int32_t *values,
                           int32_t count, csgpu_val *states_out, csgpu_result *results);

/* Convenience for single nodes with host buffers (used by the drop-in shim):
 * uploads `state` (n_vars), runs one node, downloads the result.  Synchronous. */
int csgpu_propagate_one(const csgpu_model *m, const csgpu_val *state, csgpu_node node, csgpu_val *state_out,
                        csgpu_result *result);
/* The same with the node's trail: every narrowing the fixpoint made, as {variable, 0 = lower bound raised /
 * 1 = upper bound lowered / 2 = failure seen at this variable (-1: at a constant), new bound, clause}, `clause`
 * being the index of the top-level clause (csgpu_model_num_clauses order) whose revision made it -- what the
 * reference's bind() records as binding_t.clause (csolve.h:73-79) for its conflict analysis (conflict.c:290-316).
 * trace: host, [4 * cap] int32; *count = records made (may exceed cap: the rest is lost).  Records of one round
 * are in no particular order; replaying them in sequence (intersecting) gives the fixpoint.  Runs the general
 * kernel whatever csgpu_model_set_kernel says; the order of narrowings is the device's, not the reference's
 * depth-first one, so a conflict derived from the trail is valid but not necessarily the reference's. */
int csgpu_propagate_one_traced(const csgpu_model *m, const csgpu_val *state, csgpu_node node, csgpu_val *state_out,
                               csgpu_result *result, int32_t *trace, int32_t cap, int32_t *count);
/* The trail of one node of a pure != network with the CAUSE of every bound move as a variable: records
 * {variable, 0 = lower bound raised / 1 = upper bound lowered, new bound, the valued variable whose value forbade the
 * old bound}, in the order the moves were made (one wavefront: replaying them in sequence gives the fixpoint; the
 * first record that empties a domain is the failure).  *count = moves made; at most min(cap, 2048) records are kept
 * (a longer trail is cut off: the caller sees count above that).  Runs the interval-only shaving kernel (models that qualify
 * for kernel 7, CSGPU_E_LIMIT otherwise) -- the latency of csgpu_propagate_one.  What the drop-in needs to bump the
 * variables on the way from the assignment to a failure (propagate_term_recurse, propagate.c:44-54). */
int csgpu_propagate_one_causes(const csgpu_model *m, const csgpu_val *state, csgpu_node node, csgpu_val *state_out,
                               csgpu_result *result, int32_t *trace, int32_t cap, int32_t *count);
/* The reference's OWN failure chain of one node: which variables its depth-first propagation bumps when the node fails
 * -- the variable whose domain emptied (propagate_term_confl, propagate.c:33-41; none when the failure is found at the
 * constant of an `x + c` operand) and then every variable on its recursion stack, innermost first
 * (propagate_term_recurse, propagate.c:44-54) -- and how many narrowings it made before (its PROPS of the call).  One
 * wavefront walks the reference's recursion (cs_chain.hip.h); for models whose clauses are all NOT(EQ(l, r)) with l, r a
 * variable or `variable + constant` (CSGPU_E_LIMIT otherwise).  *status = -1 (failed) or 0; bumps[0 .. min(cap, *count))
 * in the reference's order.  Tens of microseconds per node: the drop-in uses it for failing nodes only, and only when
 * asked for the reference's exact trace (CSOLVE_DROPIN_CHAIN=reference). */
int csgpu_propagate_one_chain(const csgpu_model *m, const csgpu_val *state, csgpu_node node, int32_t *status,
                              int32_t *props, int32_t *bumps, int32_t cap, int32_t *count);
/* THE RESIDENT SERVER behind the two entries above.  One propagate_clauses of the reference's driver (csolve.c:247-261)
 * is one node; as a kernel launch it costs launch submit + dispatch + completion signal + the host's wait, 14 of the
 * 19 us of a call.  For the models of kernel 7 (pure != networks of at most 256 variables) csgpu_propagate_one and
 * csgpu_propagate_one_causes therefore talk to ONE resident wavefront through a mailbox in coherent host memory: the
 * host writes node record and state, then a request number; the wave polls it, runs the fixpoint, writes state, trail
 * and result back and acknowledges.  The wave leaves when the model is freed or after 2 ms without a request
 * (CSGPU_SERVER_IDLE_US) and is started again by the next call; CSGPU_SERVER=0 keeps the launch per call.  Results are
 * those of kernel 7 (same code).  csgpu_debug_one_timing: where the host's time of these calls went -- seconds[0..3] =
 * {copy in, ring + wait, copy out, server (re)starts} with the server, {copy in, launch submit, wait for completion,
 * copy out} without; calls made, servers started. */
int csgpu_debug_one_timing(const csgpu_model *m, double *seconds, uint64_t *calls, uint64_t *starts);

#ifdef __cplusplus
}
#endif
#endif
