/* cs_search_kernels.hip.h -- the bookkeeping kernels of the search engine (cs_search.hip) and their device helpers:
 * branch, scan, emit, classify, accept, scatter, for host-driven iterations and for device-driven bursts */
#ifndef CS_SEARCH_KERNELS_HIP_H
#define CS_SEARCH_KERNELS_HIP_H

#include <hip/hip_runtime.h>
#include "../../include/csolve_gpu.h"
#include "cs_arith.h"
#include "cs_frontend.h"

#define SB 256 /* threads per block of the bookkeeping kernels */

/* device counters.  [C_SURVIVORS, C_PER_ITERATION) are zeroed at the start of every iteration (C_SKIPPED: children
 * cut without a launch, see cs_holes); C_SOLUTIONS and C_STORED run over the whole search; C_BEST holds the
 * incumbent (an int in the low half).  The solution stream is a ring of stream_cap rows; positions count the rows
 * appended since it was last emptied, position p lives at row p mod stream_cap: C_STREAM = the next free position (the
 * accept kernels take theirs there; the fused levels are given theirs by the host), C_STREAM_HEAD = the oldest
 * position not drained (a position below C_STREAM_HEAD + stream_cap is free to write), C_STREAM_ERR != 0: a kernel
 * found no room */
enum { C_SURVIVORS = 0, C_COMPLETE, C_CUTS, C_PROPS, C_REVS, C_TOTAL_CHILDREN, C_SKIPPED, C_PER_ITERATION,
       C_SOLUTIONS = C_PER_ITERATION, C_STORED, C_BEST, C_STREAM, C_STREAM_HEAD, C_STREAM_ERR, C_COUNT };

/* Values that the parent's own forbidden set already rules out (models whose states carry one set word per
 * variable): the child "variable = such a value" violates a != clause with a valued neighbour, so its fixpoint
 * can only fail.  Such children are counted as nodes and cuts but never launched: the tree, CALLS and CUTS are
 * those of enumerating every value of the interval, the batches are a fraction of it. */
struct cs_holes {
  const unsigned long long *pool_forb; /* nullptr: every value of the interval becomes a launched child */
  const int *root_lo;
  /* the branching rule (strategy_var_cmp, reference src/strategy.c:79-121): which open variable comes first --
   * order 0 none, 1 smallest domain (the default), 2 largest domain, 3 smallest value, 4 largest value -- and, with
   * `prio` != nullptr (-f true: prefer failing), among equals the one with the highest failure count; then the
   * lowest index.  What the reference keeps in a heap is the minimum of this key over the open variables. */
  int order;
  const int *prio;
};

/* the whole key: state part, then failure count (higher first), then index (cs_arith.h: the same function is
 * exported as csgpu_branch_key and pinned by the reference's VarCmp vectors) */
__device__ __forceinline__ unsigned long long cs_branch_key(const cs_holes &H, cs_val d, int v) {
  return cs_branch_key_of(H.order, H.prio != nullptr, d, H.prio != nullptr ? (long long)H.prio[v] : 0ll, v);
}

/* what the branching step decides for a parent and the emitting step needs (32 bytes per parent) */
struct cs_choice {
  int var;             /* -1: no open variable */
  int lo, hi;          /* the branching variable's interval */
  int count;           /* children that are launched */
  unsigned a_lo, a_hi; /* holes != 0: bit j <=> value lo + j is a child */
  int holes;           /* the parent's set was consulted: only the values it allows become children */
  int skipped;         /* values of the interval cut without a launch */
};

/* state of the device-driven iterations, in device memory between the kernels of a burst */
enum { B_TOP = 0, B_BUDGET, B_LIMIT, B_LIMIT_MAX, B_ITER_BASE, B_ITERS, B_NODES, B_CUTS, B_PROPS, B_REVS, B_PEAK, B_ERROR,
       B_SCATTER_BASE, B_IMPROVED, B_D_PARENTS, B_D_FIRST, B_D_ITER /* the iteration cs_burst_branch decided on */,
       B_BACKLOG_DIV /* parents = pool / this, within [B_LIMIT, B_LIMIT_MAX] */, B_COUNT };
#define BURST_ITERATIONS 16
/* a MIN / MAX iteration's bookkeeping is spread over this many workgroups (one workgroup is bound by what ONE CU
 * reads, ~25 GB/s: 1,024 parent rows took it 24 us, 10,000 results 18 us) */
#define BURST_PPW 64        /* parents per workgroup: sixteen lanes each, one pass of 1,024 threads */
#define BURST_WGS_MAX 256   /* one wave adds up the workgroups' child counts, four each: at most 16,384 parents per iteration */
#define BURST_PARENTS_MAX (BURST_PPW * BURST_WGS_MAX)
#define BURST_CLASS_WGS 128 /* at most 1,024: a workgroup adds up the others' counts one per thread */

#define SPLIT_WIDTH 256 /* wider intervals are halved instead of enumerated (csolve.c:121-150 style) */

/* the values lo .. lo + width - 1 of a variable whose set word is `forb` (bit k = value root_lo + k):
 * bit j of the result <=> value lo + j is not forbidden.  32-bit halves (no variable 64-bit shifts). */
__device__ __forceinline__ void cs_allowed_values(unsigned long long forb, int rel_lo, int width, unsigned *a_lo,
                                                  unsigned *a_hi) {
  const unsigned lo = ~(unsigned)forb, hi = ~(unsigned)(forb >> 32);
  unsigned x_lo, x_hi;
  if (rel_lo >= 32) { x_lo = hi >> (rel_lo - 32); x_hi = 0u; }
  else if (rel_lo == 0) { x_lo = lo; x_hi = hi; }
  else { x_lo = (lo >> rel_lo) | (hi << (32 - rel_lo)); x_hi = hi >> rel_lo; }
  if (width < 32) { x_lo &= (1u << width) - 1u; x_hi = 0u; }
  else if (width == 32) x_hi = 0u;
  else if (width < 64) x_hi &= (1u << (width - 32)) - 1u;
  *a_lo = x_lo;
  *a_hi = x_hi;
}

/* What a lane found among ITS variables (v = sl, sl + S, ...): the smallest key and that variable's interval.  Scan and
 * pick are separate so that a caller can have the rows of several parents in flight before it reduces any of them. */
struct cs_branch_part {
  unsigned long long best;
  cs_val d;
};

template <int S>
__device__ __forceinline__ cs_branch_part cs_branch_scan(const cs_val *__restrict__ row, int n, int sl, const cs_holes &H) {
  cs_branch_part p;
  p.best = ~0ull;
  p.d = cs_value(0);
  for (int v = sl; v < n; v += S) {
    const cs_val d = row[v];
    if (d.lo != d.hi) {
      const unsigned long long key = cs_branch_key(H, d, v);
      if (key < p.best) { p.best = key; p.d = d; }
    }
  }
  return p;
}

template <int S>
__device__ __forceinline__ cs_choice cs_branch_pick(cs_branch_part p, long long row_index, int n, const cs_holes &H) {
  unsigned long long best = p.best;
  for (int o = S / 2; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o);
    best = other < best ? other : best;
  }
  cs_choice c;
  c.var = -1; c.lo = 0; c.hi = 0; c.count = 0; c.a_lo = 0u; c.a_hi = 0u; c.holes = 0; c.skipped = 0;
  if (best == ~0ull) return c;
  const int var = (int)(best & 0xffffu);
  /* the lane that scanned the variable (v = sl + k S, so sl = var mod S) holds its interval: no second look at the row */
  cs_val d;
  d.lo = __shfl(p.d.lo, var & (S - 1), S);
  d.hi = __shfl(p.d.hi, var & (S - 1), S);
  unsigned long long forb = 0ull;
  int root = 0;
  if (H.pool_forb != nullptr) {
    forb = H.pool_forb[(size_t)row_index * n + var];
    root = H.root_lo[var];
  }
  const long long width = (long long)d.hi - (long long)d.lo + 1;
  c.var = var;
  c.lo = d.lo;
  c.hi = d.hi;
  c.count = width > SPLIT_WIDTH ? 2 : (int)width;
  const long long rel_lo = (long long)d.lo - (long long)root;
  if (H.pool_forb != nullptr && width <= 64 && rel_lo >= 0 && rel_lo + width <= 64) {
    cs_allowed_values(forb, (int)rel_lo, (int)width, &c.a_lo, &c.a_hi);
    const int allowed = __popc(c.a_lo) + __popc(c.a_hi);
    c.holes = 1;
    c.skipped = c.count - allowed;
    c.count = allowed;
  }
  return c;
}

/* S lanes (a whole wave, or a half or a quarter of one for small models) per parent: the open variable the branching
 * rule puts first (cs_branch_key: by default the smallest interval, ties lowest index -- the reference's
 * "-o smallest-domain" idea, strategy.c:85-91, as a pure function of the state).  Intervals wider than SPLIT_WIDTH are
 * halved (two children) instead of enumerated.  The same choice in every lane of the segment. */
template <int S>
__device__ __forceinline__ cs_choice cs_branch_seg(const cs_val *__restrict__ row, long long row_index, int n, int sl,
                                                   const cs_holes &H) {
  return cs_branch_pick<S>(cs_branch_scan<S>(row, n, sl, H), row_index, n, H);
}

/* a workgroup takes SB / S consecutive parents; besides var and count per parent it leaves the number of
 * children of its parents in block_sum, so that the scan that follows runs over workgroups, not parents */
template <int S>
__global__ __launch_bounds__(SB) void cs_branch(const cs_val *__restrict__ pool, long long first_row, int parents,
                                                int n, cs_choice *__restrict__ choice,
                                                int *__restrict__ block_sum, cs_holes H,
                                                int *__restrict__ block_skip) {
  constexpr int PPB = SB / S;
  __shared__ int s_cnt[PPB], s_skip[PPB];
  const int seg = threadIdx.x / S, sl = threadIdx.x & (S - 1);
  const int p = blockIdx.x * PPB + seg;
  const int pc = p < parents ? p : parents - 1; /* segments past the end redo the last parent and drop it */
  const cs_choice c = cs_branch_seg<S>(pool + (size_t)(first_row + pc) * n, first_row + pc, n, sl, H);
  if (sl == 0) {
    if (p < parents) choice[p] = c;
    s_cnt[seg] = p < parents ? c.count : 0;
    s_skip[seg] = p < parents ? c.skipped : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0, skip = 0;
    for (int i = 0; i < PPB; i++) { total += s_cnt[i]; skip += s_skip[i]; }
    block_skip[blockIdx.x] = skip; /* summed by cs_scan */
    block_sum[blockIdx.x] = total;
  }
}

/* block-wide exclusive scan of one value per thread (1024 threads): wave scan with shuffles, the 16 wave
 * totals through LDS.  Returns the exclusive prefix; *total = the sum over the block. */
__device__ __forceinline__ long long cs_block_excl_scan(long long x, long long *s_part, long long *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long incl = x;
  for (int d = 1; d < 64; d <<= 1) {
    const long long up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) s_part[wave] = incl;
  __syncthreads();
  long long before = 0, all = 0;
  for (int w = 0; w < 16; w++) {
    const long long p = s_part[w];
    before += w < wave ? p : 0;
    all += p;
  }
  __syncthreads();
  *total = all;
  return before + incl - x;
}

/* exclusive scan of count[0..items) by one block; every thread takes SCAN_PER consecutive elements of a
 * tile (vector loads), the per-thread sums go through the block scan; total -> off[items] and
 * counters[total_slot].  count and off are 16-byte aligned (hipMalloc), the tail is handled one by one. */
#define SCAN_PER 16
__global__ __launch_bounds__(1024) void cs_scan(const int *__restrict__ count, int items, int *__restrict__ off,
                                                unsigned long long *__restrict__ counters, int total_slot,
                                                const int *__restrict__ extra /* nullable: summed into extra_slot */,
                                                int extra_slot) {
  __shared__ long long s_part[16];
  long long carry = 0, extra_sum = 0;
  for (int base = 0; base < items; base += 1024 * SCAN_PER) {
    const int first = base + (int)threadIdx.x * SCAN_PER;
    int x[SCAN_PER];
    if (first + SCAN_PER <= items) {
#pragma unroll
      for (int q = 0; q < SCAN_PER / 4; q++) {
        const int4 v = ((const int4 *)(count + first))[q];
        x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < SCAN_PER; q++) x[q] = first + q < items ? count[first + q] : 0;
    }
    if (extra != nullptr) {
      if (first + SCAN_PER <= items) {
#pragma unroll
        for (int q = 0; q < SCAN_PER / 4; q++) {
          const int4 v = ((const int4 *)(extra + first))[q];
          extra_sum += (long long)v.x + v.y + v.z + v.w;
        }
      } else {
        for (int q = 0; q < SCAN_PER; q++) extra_sum += first + q < items ? extra[first + q] : 0;
      }
    }
    int sum = 0;
#pragma unroll
    for (int q = 0; q < SCAN_PER; q++) { const int v = x[q]; x[q] = sum; sum += v; } /* exclusive within the thread */
    long long total;
    const long long ex = carry + cs_block_excl_scan((long long)sum, s_part, &total);
    if (first + SCAN_PER <= items) {
#pragma unroll
      for (int q = 0; q < SCAN_PER / 4; q++)
        ((int4 *)(off + first))[q] = make_int4((int)ex + x[4 * q], (int)ex + x[4 * q + 1], (int)ex + x[4 * q + 2], (int)ex + x[4 * q + 3]);
    } else {
#pragma unroll
      for (int q = 0; q < SCAN_PER; q++)
        if (first + q < items) off[first + q] = (int)ex + x[q];
    }
    carry += total;
  }
  long long extra_total = 0;
  if (extra != nullptr) (void)cs_block_excl_scan(extra_sum, s_part, &extra_total);
  if (threadIdx.x == 0) {
    off[items] = (int)carry;
    counters[total_slot] = (unsigned long long)carry;
    if (extra != nullptr) counters[extra_slot] = (unsigned long long)extra_total;
  }
}

/* the per-block class counts of cs_classify_count: exclusive scans of the survivors and of the complete
 * children (one scan: survivors in the low half of a 64-bit word, complete children in the high half), sums
 * of cuts / propagations / revisions -> counters */
__global__ __launch_bounds__(1024) void cs_scan_classes(const int *__restrict__ block_surv, const int *__restrict__ block_comp,
                                                        const int *__restrict__ block_cuts, const int *__restrict__ block_props,
                                                        const int *__restrict__ block_revs, int blocks,
                                                        int *__restrict__ surv_off, int *__restrict__ comp_off,
                                                        unsigned long long *__restrict__ counters) {
  __shared__ long long s_part[16];
  constexpr int PER = 4;
  long long carry = 0, cuts = 0, props = 0, revs = 0;
  for (int base = 0; base < blocks; base += 1024 * PER) {
    const int first = base + (int)threadIdx.x * PER;
    long long x[PER], sum = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
      const int i = first + q;
      const bool in = i < blocks;
      const long long v = in ? (long long)block_surv[i] | ((long long)block_comp[i] << 32) : 0;
      x[q] = sum;
      sum += v;
      cuts += in ? block_cuts[i] : 0;
      props += in ? block_props[i] : 0;
      revs += in ? block_revs[i] : 0;
    }
    long long total;
    const long long ex = carry + cs_block_excl_scan(sum, s_part, &total);
#pragma unroll
    for (int q = 0; q < PER; q++) {
      const int i = first + q;
      if (i < blocks) {
        surv_off[i] = (int)((ex + x[q]) & 0xffffffffll);
        comp_off[i] = (int)((ex + x[q]) >> 32);
      }
    }
    carry += total;
  }
  long long t_cuts, t_props, t_revs;
  (void)cs_block_excl_scan(cuts, s_part, &t_cuts);
  (void)cs_block_excl_scan(props, s_part, &t_props);
  (void)cs_block_excl_scan(revs, s_part, &t_revs);
  if (threadIdx.x == 0) {
    surv_off[blocks] = (int)(carry & 0xffffffffll);
    comp_off[blocks] = (int)(carry >> 32);
    counters[C_SURVIVORS] = (unsigned long long)(carry & 0xffffffffll);
    counters[C_COMPLETE] = (unsigned long long)(carry >> 32);
    counters[C_CUTS] = (unsigned long long)t_cuts;
    counters[C_PROPS] = (unsigned long long)t_props;
    counters[C_REVS] = (unsigned long long)t_revs;
  }
}

/* S lanes write the children {var, value, value, parent_row} of one parent at nodes[beg, beg + c.count) */
template <int S>
__device__ __forceinline__ void cs_emit_seg(const cs_choice &c, long long row, int beg, csgpu_node *__restrict__ nodes,
                                            int low_values_last, unsigned scramble, int sl) {
  const int var = c.var, cnt = c.count;
  if (var < 0) return;
  const long long width = (long long)c.hi - (long long)c.lo + 1;
  unsigned h = 0u;
  if (scramble != 0u && cnt > 0) {
    /* ANY: the values are tried from a pseudo-random starting point (the reference randomises its
     * value order too: the seed of step_val, csolve.c:284,331-338).  Deterministic: a function of
     * the variable, the row and the iteration only. */
    h = (scramble ^ (unsigned)var * 2654435761u ^ (unsigned)row * 40503u);
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    h %= (unsigned)cnt;
  }
  if (c.holes) {
    /* only the values the parent's set allows (cnt of them): value lo + j is the r-th allowed one from below
     * and takes the place the r-th value has in the full enumeration below */
    for (int j = sl; j < (int)width; j += S) {
      const unsigned bit = j < 32 ? (c.a_lo >> j) & 1u : (c.a_hi >> (j - 32)) & 1u;
      if (bit == 0u) continue;
      const int r = j < 32 ? __popc(c.a_lo & ((1u << j) - 1u)) : __popc(c.a_lo) + __popc(c.a_hi & ((1u << (j - 32)) - 1u));
      const int k = scramble != 0u ? (int)(((unsigned)r + (unsigned)cnt - h) % (unsigned)cnt) : (low_values_last ? cnt - 1 - r : r);
      csgpu_node nd;
      nd.var = var;
      nd.lo = c.lo + j;
      nd.hi = c.lo + j;
      nd.parent = (int)row;
      nodes[beg + k] = nd;
    }
    return;
  }
  if (width > SPLIT_WIDTH) { /* two halves, lower half first */
    const int mid = (int)(((long long)c.lo + (long long)c.hi) >> 1);
    if (sl < 2) {
      /* the pool is LIFO and later children land higher: the half written last is explored first */
      const int lower = low_values_last ? sl == 1 : sl == 0;
      csgpu_node nd;
      nd.var = var;
      nd.lo = lower ? c.lo : mid + 1;
      nd.hi = lower ? mid : c.hi;
      nd.parent = (int)row;
      nodes[beg + sl] = nd;
    }
    return;
  }
  for (int k = sl; k < cnt; k += S) {
    csgpu_node nd;
    int value = low_values_last ? c.hi - k : c.lo + k;
    if (scramble != 0u) value = c.lo + (int)(((unsigned)k + h) % (unsigned)cnt);
    nd.var = var;
    nd.lo = value;
    nd.hi = value;
    nd.parent = (int)row;
    nodes[beg + k] = nd;
  }
}

/* same geometry as cs_branch<S>: block_off[b] = children before this workgroup's parents (the scan of
 * cs_branch's block sums), the few parents in front within the workgroup are added up directly */
template <int S>
__global__ __launch_bounds__(SB) void cs_emit(long long first_row, int parents, const cs_choice *__restrict__ choice,
                                              const int *__restrict__ block_off, csgpu_node *__restrict__ nodes,
                                              int low_values_last, unsigned scramble) {
  constexpr int PPB = SB / S;
  __shared__ cs_choice s_choice[PPB];
  const int seg = threadIdx.x / S, sl = threadIdx.x & (S - 1);
  const int p0 = blockIdx.x * PPB, p = p0 + seg;
  if ((int)threadIdx.x < PPB) {
    cs_choice c;
    c.var = -1; c.lo = 0; c.hi = 0; c.count = 0; c.a_lo = 0u; c.a_hi = 0u; c.holes = 0; c.skipped = 0;
    if (p0 + (int)threadIdx.x < parents) c = choice[p0 + threadIdx.x];
    s_choice[threadIdx.x] = c;
  }
  __syncthreads();
  if (p >= parents) return;
  int beg = block_off[blockIdx.x];
  for (int j = 0; j < seg; j++) beg += s_choice[j].count;
  cs_emit_seg<S>(s_choice[seg], first_row + p, beg, nodes, low_values_last, scramble, sl);
}

/* ---- small iterations (at most SMALL_PARENTS parents: always for ANY / MIN / MAX): one workgroup does what
 * cs_branch + cs_scan + cs_emit do, and leaves the number of children on the device, so that the host need not
 * read anything before it launches the fixpoint ---- */
#define SMALL_PARENTS 1024 /* one workgroup of 1,024 threads scans their child counts */
/* the expansion of up to SMALL_PARENTS parents by one workgroup of 1,024 threads: branch, block-scan the child counts,
 * emit.  The caller's LDS: s_choice[SMALL_PARENTS], s_off[SMALL_PARENTS], s_part[16].  Leaves the numbers of children
 * in counters; BURST (cs_expand_burst): also moves the pool top, the iteration budget and the totals in `burst` */
template <bool BURST>
__device__ __forceinline__ void cs_expand_block(const cs_val *pool, long long first_row, int parents, int n,
                                                csgpu_node *nodes, unsigned long long *counters, unsigned long long *burst,
                                                int low_values_last, unsigned scramble, const cs_holes &H,
                                                cs_choice *s_choice, int *s_off, long long *s_part) {
  /* sixteen lanes per parent, 64 parents per pass of the workgroup, four passes' rows in flight at a time (measured
   * no faster than one pass at a time: 1,024 parent rows are 300 KB through ONE CU, ~25 GB/s -- 12 us whatever the order) */
  for (int p0 = (int)threadIdx.x >> 4; p0 < parents; p0 += 256) {
    cs_branch_part part[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int p = p0 + 64 * k < parents ? p0 + 64 * k : parents - 1;
      part[k] = cs_branch_scan<16>(pool + (size_t)(first_row + p) * n, n, (int)threadIdx.x & 15, H);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int p = p0 + 64 * k;
      const cs_choice c = cs_branch_pick<16>(part[k], first_row + (p < parents ? p : parents - 1), n, H);
      if ((threadIdx.x & 15) == 0 && p < parents) s_choice[p] = c;
    }
  }
  __syncthreads();
  long long total, skipped_total;
  const int t = (int)threadIdx.x;
  (void)cs_block_excl_scan(t < parents ? (long long)s_choice[t].skipped : 0, s_part, &skipped_total);
  const long long ex = cs_block_excl_scan(t < parents ? (long long)s_choice[t].count : 0, s_part, &total);
  if (t < parents) s_off[t] = (int)ex;
  if (t == 0) {
    counters[C_TOTAL_CHILDREN] = (unsigned long long)total;
    counters[C_SKIPPED] = (unsigned long long)skipped_total;
    if (BURST) {
      burst[B_TOP] = (unsigned long long)first_row;
      burst[B_ITERS] += 1ull;
      burst[B_BUDGET] -= 1ull;
      burst[B_NODES] += (unsigned long long)(total + skipped_total);
      burst[B_CUTS] += (unsigned long long)skipped_total;
    }
  }
  __syncthreads();
  for (int p = (int)threadIdx.x >> 4; p < parents; p += 64)
    cs_emit_seg<16>(s_choice[p], first_row + p, s_off[p], nodes, low_values_last, scramble, (int)threadIdx.x & 15);
}

__global__ __launch_bounds__(1024) void cs_expand_small(const cs_val *__restrict__ pool, long long first_row, int parents,
                                                        int n, csgpu_node *__restrict__ nodes,
                                                        unsigned long long *__restrict__ counters, int low_values_last,
                                                        unsigned scramble, cs_holes H) {
  __shared__ cs_choice s_choice[SMALL_PARENTS];
  __shared__ int s_off[SMALL_PARENTS];
  __shared__ long long s_part[16];
  if (threadIdx.x < C_PER_ITERATION) counters[threadIdx.x] = 0ull;
  cs_expand_block<false>(pool, first_row, parents, n, nodes, counters, nullptr, low_values_last, scramble, H, s_choice,
                         s_off, s_part);
}


/* Classification of the children, deterministic: pool rows and the order of the solution check
 * depend on the child index only (block counts -> exclusive scan -> rows), never on which
 * workgroup finished first, so a search is reproducible run to run. */
__global__ __launch_bounds__(SB) void cs_classify_count(const csgpu_result *__restrict__ res, int children,
                                                        int *__restrict__ block_surv, int *__restrict__ block_comp,
                                                        int *__restrict__ block_cuts, int *__restrict__ block_props,
                                                        int *__restrict__ block_revs) {
  __shared__ int s_sum[5][SB / 64];
  const int t = threadIdx.x, i = blockIdx.x * SB + t;
  int status = -2, props = 0, revs = 0;
  if (i < children) {
    status = res[i].status;
    props = status >= 0 ? res[i].props : 0; /* propagations of consistent children only: on a != network those are the
                                             * reference's PROPS; an inconsistent child's count depends on the revision order */
    revs = res[i].revisions;
  }
  int ps = status > 0, pk = status == 0, pc = status == -1, pp = props, pr = revs;
  for (int o = 32; o > 0; o >>= 1) {
    ps += __shfl_xor(ps, o);
    pk += __shfl_xor(pk, o);
    pc += __shfl_xor(pc, o);
    pp += __shfl_xor(pp, o);
    pr += __shfl_xor(pr, o);
  }
  if ((t & 63) == 0) {
    s_sum[0][t >> 6] = ps; s_sum[1][t >> 6] = pk; s_sum[2][t >> 6] = pc; s_sum[3][t >> 6] = pp; s_sum[4][t >> 6] = pr;
  }
  __syncthreads();
  if (t < 5) {
    int v = 0;
    for (int w = 0; w < SB / 64; w++) v += s_sum[t][w];
    int *dst = t == 0 ? block_surv : (t == 1 ? block_comp : (t == 2 ? block_cuts : (t == 3 ? block_props : block_revs)));
    dst[blockIdx.x] = v; /* folded by cs_scan_classes: sums do not depend on any order */
  }
}

__global__ __launch_bounds__(SB) void cs_classify_assign(const csgpu_result *__restrict__ res, int children,
                                                         const int *__restrict__ surv_off,
                                                         const int *__restrict__ comp_off, int *__restrict__ surv_list,
                                                         int *__restrict__ complete_list) {
  __shared__ int s_surv[SB], s_comp[SB];
  const int t = threadIdx.x, i = blockIdx.x * SB + t;
  const int status = i < children ? res[i].status : -2;
  const int surv = status > 0, comp = status == 0;
  s_surv[t] = surv;
  s_comp[t] = comp;
  __syncthreads();
  for (int d = 1; d < SB; d <<= 1) {
    int a = t >= d ? s_surv[t - d] : 0, b = t >= d ? s_comp[t - d] : 0;
    __syncthreads();
    s_surv[t] += a;
    s_comp[t] += b;
    __syncthreads();
  }
  if (i < children) {
    if (surv) surv_list[surv_off[blockIdx.x] + s_surv[t] - 1] = i; /* survivor k goes to pool row new_top + k */
    if (comp) complete_list[comp_off[blockIdx.x] + s_comp[t] - 1] = i;
  }
}

/* -f true (prefer failing): the failure counts the branching rule looks at.  What the reference does per node
 * (csolve.c:455-465: the branching variable's prio-- when its assignment holds, prio++ when it fails;
 * propagate_term_confl, propagate.c:33-41: prio++ of the variable whose domain emptied), for a whole batch of children.
 * The reference's further bumps along its recursion stack (propagate.c:44-54) follow its depth-first order and have
 * no counterpart in a batch.  fail_var_known: the fixpoint kernel reports the emptied variable in result.rounds. */
/* prio[var] += delta for the lanes with var >= 0, ONE atomic per distinct variable of the wave: the children of a parent
 * share their variable and most failures empty the same one, so a lane each was 130,000 atomics on one word per
 * iteration of schedule-12 -- 1.5 ms at the ~88 atomics per microsecond a word sustains (2.3 ms per iteration with -f
 * true against 0.14 without) */
__device__ __forceinline__ void cs_wave_bump(int *__restrict__ prio, int var, int delta) {
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long todo = __ballot(var >= 0);
  while (todo != 0ull) {
    const int leader = __builtin_ctzll(todo);
    const int lv = __builtin_amdgcn_readlane(var, leader);
    const unsigned long long same = __ballot(var == lv);
    const int sum = __popcll(__ballot(var == lv && delta > 0)) - __popcll(__ballot(var == lv && delta < 0));
    if (lane == leader && sum != 0) atomicAdd(&prio[lv], sum);
    todo &= ~same;
  }
}

__global__ __launch_bounds__(SB) void cs_prio_update(const csgpu_result *__restrict__ res, const csgpu_node *__restrict__ nodes,
                                                     int children, const unsigned long long *__restrict__ children_dev,
                                                     int n, int fail_var_known, int *__restrict__ prio) {
  if (children_dev != nullptr && (long long)*children_dev < (long long)children) children = (int)*children_dev;
  const int i = blockIdx.x * SB + threadIdx.x;
  if ((int)(blockIdx.x * SB) >= children) return; /* uniform over the workgroup; the waves below stay whole */
  int v = -1, failed_on = -1, delta = 0;
  if (i < children) {
    const csgpu_result r = res[i];
    v = nodes[i].var;
    if (v < 0 || v >= n) v = -1;
    delta = r.status >= 0 ? -1 : 1;
    if (v >= 0 && r.status < 0 && fail_var_known && r.rounds >= 0 && r.rounds < n && r.rounds != v) failed_on = r.rounds;
  }
  cs_wave_bump(prio, v, delta);
  cs_wave_bump(prio, failed_on, 1);
}

/* small iterations: cs_classify_count + cs_scan_classes + cs_classify_assign in one workgroup, the number of
 * children read from the device.  Same rows and the same order as the large path (tiles in child order). */
__global__ __launch_bounds__(1024) void cs_classify_small(const csgpu_result *__restrict__ res,
                                                          int *__restrict__ surv_list, int *__restrict__ complete_list,
                                                          unsigned long long *__restrict__ counters,
                                                          unsigned long long *__restrict__ burst) {
  __shared__ long long s_part[16];
  const int children = (int)counters[C_TOTAL_CHILDREN];
  long long carry = 0; /* survivors in the low half, complete children in the high half: one scan for both */
  long long cuts = 0, props = 0, revs = 0; /* per thread, reduced once at the end */
  /* consecutive children per thread and tile (sixteen, so that a MIN iteration of 10,000 children is one tile, was
   * measured no faster: this single workgroup is bound by what ONE CU reads, ~25 GB/s -- 160 KB of results are 7 us) */
  constexpr int PER = 4;
  for (int base = 0; base < children; base += 1024 * PER) {
    const int first = base + (int)threadIdx.x * PER;
    int status[PER];
    long long sum = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
      const int i = first + q;
      status[q] = -2;
      if (i < children) {
        const csgpu_result r = res[i];
        status[q] = r.status;
        props += r.status >= 0 ? r.props : 0;
        revs += r.revisions;
        cuts += r.status == -1;
      }
      sum += (long long)(status[q] > 0) | ((long long)(status[q] == 0) << 32);
    }
    long long total;
    long long ex = carry + cs_block_excl_scan(sum, s_part, &total);
#pragma unroll
    for (int q = 0; q < PER; q++) {
      if (status[q] > 0) surv_list[ex & 0xffffffffll] = first + q;
      if (status[q] == 0) complete_list[ex >> 32] = first + q;
      ex += (long long)(status[q] > 0) | ((long long)(status[q] == 0) << 32);
    }
    carry += total;
  }
  long long t_cuts, t_props, t_revs;
  (void)cs_block_excl_scan(cuts, s_part, &t_cuts);
  (void)cs_block_excl_scan(props, s_part, &t_props);
  (void)cs_block_excl_scan(revs, s_part, &t_revs);
  if (threadIdx.x == 0) {
    counters[C_SURVIVORS] = (unsigned long long)(carry & 0xffffffffll);
    counters[C_COMPLETE] = (unsigned long long)(carry >> 32);
    counters[C_CUTS] = (unsigned long long)t_cuts;
    counters[C_PROPS] = (unsigned long long)t_props;
    counters[C_REVS] = (unsigned long long)t_revs;
    if (burst != nullptr) { /* device-driven iterations: the pool top and the running totals live on the device */
      const unsigned long long base = burst[B_TOP], top = base + (unsigned long long)(carry & 0xffffffffll);
      burst[B_SCATTER_BASE] = base;
      burst[B_TOP] = top;
      if (top > burst[B_PEAK]) burst[B_PEAK] = top;
      burst[B_CUTS] += (unsigned long long)t_cuts;
      burst[B_PROPS] += (unsigned long long)t_props;
      burst[B_REVS] += (unsigned long long)t_revs;
    }
  }
}

/* the next free position of the solution stream for `rows` rows, and ring row of position `at`: -1 and the error flag
 * when they would overwrite rows not yet drained (the host sizes the iterations so that this never happens) */
__device__ __forceinline__ long long cs_stream_take(unsigned long long *__restrict__ counters, unsigned long long at,
                                                    unsigned rows, long long stream_cap) {
  if (at + rows > counters[C_STREAM_HEAD] + (unsigned long long)stream_cap) {
    counters[C_STREAM_ERR] = 1ull;
    return -1;
  }
  return (long long)(at % (unsigned long long)stream_cap);
}

/* cs_accept + cs_pick_best for the complete children of a small iteration, by one workgroup, nothing read by the
 * host: counts the solutions, moves the incumbent, keeps a state that attains it (and, ANY: the first one).
 * Called by every thread of a workgroup of at least 256 threads (the first 256 work; uniform control flow). */
__device__ __forceinline__ void cs_accept_block(const cs_val *__restrict__ child_states, const int *__restrict__ list,
                                                const int *__restrict__ truth, int n, int objective, int obj_var,
                                                unsigned long long *__restrict__ counters,
                                                unsigned long long *__restrict__ burst, int32_t *__restrict__ solutions,
                                                long long max_solutions, int32_t *__restrict__ best_solution,
                                                int *__restrict__ best /* the incumbent: may be shared between engines */,
                                                int32_t *__restrict__ stream /* nullable: the picked row is appended */,
                                                long long stream_cap) {
  __shared__ long long s_key[256];
  __shared__ int s_cnt[256];
  __shared__ int s_pick;
  __shared__ long long s_slot;
  const int count = (int)counters[C_COMPLETE];
  if (count == 0) return; /* uniform */
  const int t = (int)threadIdx.x;
  const bool opt = objective == CS_OBJ_MIN || objective == CS_OBJ_MAX;
  /* key: (objective value, made "smaller is better") << 32 | child index: the minimum is the best value and,
   * among equals, the first child */
  long long key = 0x7fffffffffffffffll;
  int cnt = 0;
  if (t < 256)
    for (int i = t; i < count; i += 256) {
      if (truth != nullptr && truth[i] != 1) continue; /* truth == NULL: every complete child is a solution */
      cnt++;
      long long val = 0;
      if (opt) {
        const cs_val o = child_states[(size_t)list[i] * n + obj_var];
        val = objective == CS_OBJ_MIN ? (long long)o.lo : -(long long)o.hi;
      }
      const long long k = val * 4294967296ll + (long long)i;
      key = k < key ? k : key;
      if (objective != CS_OBJ_ANY && counters[C_STORED] < (unsigned long long)max_solutions) {
        const unsigned long long slot = atomicAdd(&counters[C_STORED], 1ull);
        if (slot < (unsigned long long)max_solutions)
          for (int v = 0; v < n; v++) solutions[(size_t)slot * n + v] = child_states[(size_t)list[i] * n + v].lo;
      }
    }
  if (t < 256) {
    s_key[t] = key;
    s_cnt[t] = cnt;
  }
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (t < d) {
      s_key[t] = s_key[t + d] < s_key[t] ? s_key[t + d] : s_key[t];
      s_cnt[t] += s_cnt[t + d];
    }
    __syncthreads();
  }
  if (t == 0) {
    s_pick = -1;
    s_slot = -1;
    const int accepted = s_cnt[0];
    if (accepted > 0) {
      const long long best_key = s_key[0];
      const int idx = (int)(best_key & 0xffffffffll);
      if (objective == CS_OBJ_ANY) {
        /* found_any (csolve.c:207-209): exactly one solution is accepted, the first in child order */
        if (counters[C_STORED] == 0ull) {
          counters[C_SOLUTIONS] += 1ull;
          counters[C_STORED] = 1ull;
          s_pick = idx;
        }
      } else {
        counters[C_SOLUTIONS] += (unsigned long long)accepted;
        if (opt) {
          const long long v = (best_key - (long long)idx) / 4294967296ll;
          const int val = objective == CS_OBJ_MIN ? (int)v : (int)-v;
          /* atomic: engines that share the incumbent accept concurrently */
          const int old = objective == CS_OBJ_MIN ? atomicMin(best, val) : atomicMax(best, val);
          if (objective == CS_OBJ_MIN ? val < old : val > old) {
            burst[B_IMPROVED] = 0x100000000ull | (unsigned)val; /* flag | the value the stored row attains */
            s_pick = idx;
          }
        }
      }
    }
    /* the stream takes the picked row too (ANY: the one solution; MIN / MAX: the one that improved the incumbent);
     * one workgroup, one row: the slot is this thread's to take */
    if (stream != nullptr && s_pick >= 0) {
      const unsigned long long at = counters[C_STREAM];
      s_slot = cs_stream_take(counters, at, 1u, stream_cap);
      if (s_slot >= 0) counters[C_STREAM] = at + 1ull;
    }
  }
  __syncthreads();
  const int pick = s_pick;
  if (pick >= 0 && t < 256) {
    int32_t *out = objective == CS_OBJ_ANY ? solutions : best_solution;
    const long long slot = s_slot;
    for (int v = t; v < n; v += 256) {
      const int32_t x = child_states[(size_t)list[pick] * n + v].lo;
      out[v] = x;
      if (slot >= 0) stream[(size_t)slot * n + v] = x;
    }
  }
  __syncthreads();
}

/* the accept of the LAST iteration of a burst (the others run at the head of the next cs_expand_burst) */
__global__ __launch_bounds__(256) void cs_accept_burst(const cs_val *__restrict__ child_states, const int *__restrict__ list,
                                                       const int *__restrict__ truth, int n, int objective, int obj_var,
                                                       unsigned long long *__restrict__ counters,
                                                       unsigned long long *__restrict__ burst,
                                                       int32_t *__restrict__ solutions, long long max_solutions,
                                                       int32_t *__restrict__ best_solution, int *__restrict__ best,
                                                       int32_t *__restrict__ stream, long long stream_cap) {
  cs_accept_block(child_states, list, truth, n, objective, obj_var, counters, burst, solutions, max_solutions, best_solution,
                  best, stream, stream_cap);
  if (threadIdx.x == 0) counters[C_COMPLETE] = 0ull; /* accepted: the next burst's first expansion must not do it again */
}

/* the head of a device-driven iteration -- how many parents, from which row -- as a function of `burst` alone, so
 * that every workgroup of a split expansion can decide it for itself */
struct cs_burst_head {
  int parents, error;
  long long first_row, iter;
};
__device__ __forceinline__ cs_burst_head cs_burst_decide(const unsigned long long *__restrict__ burst, bool done,
                                                         long long max_width, long long cap, long long room_limit) {
  cs_burst_head h;
  h.error = 0;
  const long long top = (long long)burst[B_TOP];
  /* a few parents while the pool is small (dive for a solution / an incumbent first), more once there is a
   * backlog of open states: a share of the pool (B_BACKLOG_DIV), within [B_LIMIT, B_LIMIT_MAX] (schedule-10: 0.7 s
   * instead of 1.6 s with 64 throughout; small searches lose a few ms) */
  long long limit = top / (long long)burst[B_BACKLOG_DIV];
  limit = limit < (long long)burst[B_LIMIT] ? (long long)burst[B_LIMIT] : limit;
  limit = limit > (long long)burst[B_LIMIT_MAX] ? (long long)burst[B_LIMIT_MAX] : limit;
  long long parents = top < limit ? top : limit;
  if (burst[B_BUDGET] == 0ull || burst[B_ERROR] != 0ull || done) parents = 0;
  if (parents > 0 && top - parents + parents * max_width > room_limit) { /* as one_iteration */
    const long long fit = max_width > 1 ? (room_limit - top) / (max_width - 1) : parents;
    parents = fit < 1 ? 1 : (fit < parents ? fit : parents);
    if (top - parents + parents * max_width > cap) {
      h.error = 1;
      parents = 0;
    }
  }
  h.parents = (int)parents;
  h.first_row = top - parents;
  h.iter = (long long)(burst[B_ITER_BASE] + burst[B_ITERS]);
  return h;
}

/* ---- device-driven iterations: what the host does around a small iteration, on the device ----
 * cs_expand_burst = the head of one_iteration (how many parents, does it fit) + cs_expand_small; the pool top,
 * the iteration budget and the running totals are in `burst`.  An iteration with nothing to do (pool empty,
 * budget used up, ANY already solved, error) leaves zero children, and every later kernel of it returns at once. */
__global__ __launch_bounds__(1024) void cs_expand_burst(const cs_val *__restrict__ pool, int n, csgpu_node *__restrict__ nodes,
                                                        unsigned long long *__restrict__ counters,
                                                        unsigned long long *__restrict__ burst, int objective,
                                                        long long max_width, long long cap, long long room_limit,
                                                        cs_holes H, const cs_val *__restrict__ child_states,
                                                        const int *__restrict__ complete_list,
                                                        const int *__restrict__ truth, int obj_var,
                                                        int32_t *__restrict__ solutions, long long max_solutions,
                                                        int32_t *__restrict__ best_solution, int *__restrict__ best,
                                                        int32_t *__restrict__ stream, long long stream_cap) {
  __shared__ cs_choice s_choice[SMALL_PARENTS];
  __shared__ int s_off[SMALL_PARENTS];
  __shared__ long long s_part[16];
  __shared__ long long s_first, s_iter;
  __shared__ int s_parents;
  /* first the accept of the previous iteration's complete children (their root evaluation has run): it decides
   * whether ANY is done and moves the incumbent this iteration's fixpoints will see */
  cs_accept_block(child_states, complete_list, truth, n, objective, obj_var, counters, burst, solutions, max_solutions,
                  best_solution, best, stream, stream_cap);
  if (threadIdx.x == 0) {
    const cs_burst_head h = cs_burst_decide(burst, objective == CS_OBJ_ANY && counters[C_STORED] != 0ull, max_width, cap, room_limit);
    if (h.error) burst[B_ERROR] = 1ull;
    s_parents = h.parents;
    s_first = h.first_row;
    s_iter = h.iter;
  }
  if (threadIdx.x < C_PER_ITERATION) counters[threadIdx.x] = 0ull;
  __syncthreads();
  const int parents = s_parents;
  if (parents == 0) return;
  const long long first_row = s_first;
  const int low_values_last = objective == CS_OBJ_MAX ? 0 : 1;
  const unsigned scramble =
      objective == CS_OBJ_ANY ? (unsigned)((unsigned long long)s_iter * 2654435761ull + 0x9e3779b9u) | 1u : 0u;
  cs_expand_block<true>(pool, first_row, parents, n, nodes, counters, burst, low_values_last, scramble, H, s_choice,
                        s_off, s_part);
}

/* ---- the same iteration by up to BURST_WGS_MAX workgroups (MIN / MAX, whose iterations take 1,024 parents and more) ----
 * cs_burst_branch: workgroup g chooses for parents [64 g, 64 g + 64) and leaves their child counts' sum; workgroup 0
 * also runs the previous iteration's accept and publishes the head.  Nothing any workgroup READS to decide the head
 * is written here (the accept touches the incumbent, the solution counters and B_IMPROVED only), so all of them
 * decide alike without waiting for one another.
 * cs_burst_emit: workgroup g adds up its predecessors' sums (sixteen numbers) and writes its parents' children;
 * workgroup 0 moves the pool top and the running totals.  Same nodes in the same places as cs_expand_burst. */
__global__ __launch_bounds__(1024) void cs_burst_branch(const cs_val *__restrict__ pool, int n,
                                                        unsigned long long *__restrict__ counters,
                                                        unsigned long long *__restrict__ burst, int objective,
                                                        long long max_width, long long cap, long long room_limit,
                                                        cs_holes H, cs_choice *__restrict__ choice,
                                                        int *__restrict__ wg_sum, int *__restrict__ wg_skip,
                                                        const cs_val *__restrict__ child_states,
                                                        const int *__restrict__ complete_list,
                                                        const int *__restrict__ truth, int obj_var,
                                                        int32_t *__restrict__ solutions, long long max_solutions,
                                                        int32_t *__restrict__ best_solution, int *__restrict__ best,
                                                        int32_t *__restrict__ stream, long long stream_cap) {
  __shared__ int s_cnt[BURST_PPW], s_skip[BURST_PPW];
  __shared__ long long s_first;
  __shared__ int s_parents;
  const int g = (int)blockIdx.x;
  if (g == 0) /* uniform within the workgroup */
    cs_accept_block(child_states, complete_list, truth, n, objective, obj_var, counters, burst, solutions, max_solutions,
                    best_solution, best, stream, stream_cap);
  if (threadIdx.x == 0) {
    const cs_burst_head h = cs_burst_decide(burst, false, max_width, cap, room_limit);
    s_parents = h.parents;
    s_first = h.first_row;
    if (g == 0) {
      if (h.error) burst[B_ERROR] = 1ull;
      burst[B_D_PARENTS] = (unsigned long long)h.parents;
      burst[B_D_FIRST] = (unsigned long long)h.first_row;
      burst[B_D_ITER] = (unsigned long long)h.iter;
    }
  }
  if (g == 0 && threadIdx.x < C_PER_ITERATION) counters[threadIdx.x] = 0ull;
  __syncthreads();
  const int parents = s_parents;
  const int p = g * BURST_PPW + ((int)threadIdx.x >> 4);
  if (g * BURST_PPW >= parents) { /* uniform */
    if (threadIdx.x == 0) { wg_sum[g] = 0; wg_skip[g] = 0; }
    return;
  }
  const long long first_row = s_first;
  const int pc = p < parents ? p : parents - 1;
  const cs_choice c = cs_branch_seg<16>(pool + (size_t)(first_row + pc) * n, first_row + pc, n, (int)threadIdx.x & 15, H);
  if ((threadIdx.x & 15) == 0) {
    if (p < parents) choice[p] = c;
    s_cnt[threadIdx.x >> 4] = p < parents ? c.count : 0;
    s_skip[threadIdx.x >> 4] = p < parents ? c.skipped : 0;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    int cnt = s_cnt[threadIdx.x], skip = s_skip[threadIdx.x];
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o); skip += __shfl_xor(skip, o); }
    if (threadIdx.x == 0) { wg_sum[g] = cnt; wg_skip[g] = skip; }
  }
}

__global__ __launch_bounds__(1024) void cs_burst_emit(csgpu_node *__restrict__ nodes,
                                                      unsigned long long *__restrict__ counters,
                                                      unsigned long long *__restrict__ burst, int objective,
                                                      const cs_choice *__restrict__ choice,
                                                      const int *__restrict__ wg_sum, const int *__restrict__ wg_skip) {
  const int wgs = (int)gridDim.x; /* <= BURST_WGS_MAX */
  __shared__ cs_choice s_choice[BURST_PPW];
  __shared__ int s_off[BURST_PPW];
  const int g = (int)blockIdx.x;
  const int parents = (int)burst[B_D_PARENTS];
  if (g * BURST_PPW >= parents) return; /* uniform; parents == 0: the counters are zero already, nothing moves */
  const long long first_row = (long long)burst[B_D_FIRST];
  const long long iter = (long long)burst[B_D_ITER];
  if (threadIdx.x < 64) {
    const int t = (int)threadIdx.x, p = g * BURST_PPW + t;
    cs_choice c;
    c.var = -1; c.lo = 0; c.hi = 0; c.count = 0; c.a_lo = 0u; c.a_hi = 0u; c.holes = 0; c.skipped = 0;
    if (p < parents) c = choice[p];
    s_choice[t] = c;
    /* the children before this workgroup's parents, then before this parent */
    int before = 0, all = 0, all_skip = 0;
    for (int h = t; h < wgs; h += 64) {
      const int sum = wg_sum[h];
      before += h < g ? sum : 0;
      all += sum;
      all_skip += wg_skip[h];
    }
    int incl = c.count;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (t >= d) incl += up;
    }
    for (int o = 32; o > 0; o >>= 1) {
      before += __shfl_xor(before, o);
      all += __shfl_xor(all, o);
      all_skip += __shfl_xor(all_skip, o);
    }
    s_off[t] = before + incl - c.count;
    if (g == 0 && t == 0) {
      counters[C_TOTAL_CHILDREN] = (unsigned long long)all;
      counters[C_SKIPPED] = (unsigned long long)all_skip;
      burst[B_TOP] = (unsigned long long)first_row;
      burst[B_ITERS] += 1ull;
      burst[B_BUDGET] -= 1ull;
      burst[B_NODES] += (unsigned long long)((long long)all + all_skip);
      burst[B_CUTS] += (unsigned long long)all_skip;
    }
  }
  __syncthreads();
  const int low_values_last = objective == CS_OBJ_MAX ? 0 : 1;
  const unsigned scramble =
      objective == CS_OBJ_ANY ? (unsigned)((unsigned long long)iter * 2654435761ull + 0x9e3779b9u) | 1u : 0u;
  const int q = (int)threadIdx.x >> 4;
  if (g * BURST_PPW + q < parents)
    cs_emit_seg<16>(s_choice[q], first_row + g * BURST_PPW + q, s_off[q], nodes, low_values_last, scramble, (int)threadIdx.x & 15);
}

/* cs_classify_small by BURST_CLASS_WGS workgroups: cs_burst_count leaves each workgroup's class counts (its share is
 * children / BURST_CLASS_WGS consecutive children), cs_burst_assign adds up its predecessors' and writes the lists in
 * child order, copies ITS survivors into the pool (no cs_scatter launch); its workgroup 0 moves the pool top and the
 * totals. */
__device__ __forceinline__ void cs_burst_share(int children, int g, int *beg, int *end) {
  const int chunk = (children + BURST_CLASS_WGS - 1) / BURST_CLASS_WGS;
  const long long b = (long long)g * chunk, e = b + chunk;
  *beg = b < children ? (int)b : children;
  *end = e < children ? (int)e : children;
}

__global__ __launch_bounds__(1024) void cs_burst_count(const csgpu_result *__restrict__ res,
                                                       const unsigned long long *__restrict__ counters,
                                                       int *__restrict__ wg_surv, int *__restrict__ wg_comp,
                                                       int *__restrict__ wg_cuts, int *__restrict__ wg_props,
                                                       int *__restrict__ wg_revs) {
  __shared__ long long s_part[16];
  int beg, end;
  cs_burst_share((int)counters[C_TOTAL_CHILDREN], (int)blockIdx.x, &beg, &end);
  long long classes = 0, cuts = 0, props = 0, revs = 0;
  for (int i = beg + (int)threadIdx.x; i < end; i += 1024) {
    const csgpu_result r = res[i];
    classes += (long long)(r.status > 0) | ((long long)(r.status == 0) << 32);
    props += r.status >= 0 ? r.props : 0;
    revs += r.revisions;
    cuts += r.status == -1;
  }
  long long t_classes, t_cuts, t_props, t_revs;
  (void)cs_block_excl_scan(classes, s_part, &t_classes);
  (void)cs_block_excl_scan(cuts, s_part, &t_cuts);
  (void)cs_block_excl_scan(props, s_part, &t_props);
  (void)cs_block_excl_scan(revs, s_part, &t_revs);
  if (threadIdx.x == 0) {
    wg_surv[blockIdx.x] = (int)(t_classes & 0xffffffffll);
    wg_comp[blockIdx.x] = (int)(t_classes >> 32);
    wg_cuts[blockIdx.x] = (int)t_cuts;
    wg_props[blockIdx.x] = (int)t_props;
    wg_revs[blockIdx.x] = (int)t_revs;
  }
}

__global__ __launch_bounds__(1024) void cs_burst_assign(const csgpu_result *__restrict__ res,
                                                        int *__restrict__ surv_list, int *__restrict__ complete_list,
                                                        unsigned long long *__restrict__ counters,
                                                        unsigned long long *__restrict__ burst,
                                                        const int *__restrict__ wg_surv, const int *__restrict__ wg_comp,
                                                        const int *__restrict__ wg_cuts, const int *__restrict__ wg_props,
                                                        const int *__restrict__ wg_revs,
                                                        const cs_val *__restrict__ child_states, cs_val *__restrict__ pool,
                                                        int n, const unsigned long long *__restrict__ child_forb,
                                                        unsigned long long *__restrict__ pool_forb, int fw) {
  __shared__ long long s_part[16];
  const int g = (int)blockIdx.x;
  int beg, end;
  cs_burst_share((int)counters[C_TOTAL_CHILDREN], g, &beg, &end);
  /* survivors | complete children << 32 of every workgroup, one per thread: the sum of the predecessors' and of all */
  const int t = (int)threadIdx.x;
  const long long mine = t < BURST_CLASS_WGS ? (long long)wg_surv[t] | ((long long)wg_comp[t] << 32) : 0ll;
  long long carry, classes_all;
  (void)cs_block_excl_scan(t < g ? mine : 0ll, s_part, &carry);
  (void)cs_block_excl_scan(mine, s_part, &classes_all);
  const int first_surv = (int)(carry & 0xffffffffll);
  for (int base = beg; base < end; base += 1024) {
    const int i = base + (int)threadIdx.x;
    const int status = i < end ? res[i].status : -2;
    const long long x = (long long)(status > 0) | ((long long)(status == 0) << 32);
    long long total;
    const long long ex = carry + cs_block_excl_scan(x, s_part, &total);
    if (status > 0) surv_list[ex & 0xffffffffll] = i;
    if (status == 0) complete_list[ex >> 32] = i;
    carry += total;
  }
  /* cs_scatter for this workgroup's survivors: rows first_surv .. of the new pool top (the rows of the iteration's
   * parents, B_D_FIRST, are the first to be overwritten: LIFO), walked flat so that small models fill the lanes */
  const int here = (int)(carry & 0xffffffffll) - first_surv;
  if (here > 0) { /* uniform */
    __syncthreads(); /* this workgroup's part of surv_list is written */
    const long long row0 = (long long)burst[B_D_FIRST] + first_surv;
    const int *src = surv_list + first_surv;
    {
      const int total = here * n;
      int c = (int)threadIdx.x / n, v = (int)threadIdx.x - c * n;
      const int dc = 1024 / n, dv = 1024 - dc * n;
      cs_val *dst = pool + (size_t)row0 * n;
      for (int e = (int)threadIdx.x; e < total; e += 1024) {
        dst[e] = child_states[(size_t)src[c] * n + v];
        c += dc; v += dv;
        if (v >= n) { v -= n; c++; }
      }
    }
    if (fw > 0) {
      const int nf = n * fw, total = here * nf;
      int c = (int)threadIdx.x / nf, k = (int)threadIdx.x - c * nf;
      const int dc = 1024 / nf, dk = 1024 - dc * nf;
      unsigned long long *dst = pool_forb + (size_t)row0 * nf;
      for (int e = (int)threadIdx.x; e < total; e += 1024) {
        dst[e] = child_forb[(size_t)src[c] * nf + k];
        c += dc; k += dk;
        if (k >= nf) { k -= nf; c++; }
      }
    }
  }
  if (g != 0) return; /* uniform */
  long long cuts, props, revs;
  (void)cs_block_excl_scan(t < BURST_CLASS_WGS ? (long long)wg_cuts[t] : 0ll, s_part, &cuts);
  (void)cs_block_excl_scan(t < BURST_CLASS_WGS ? (long long)wg_props[t] : 0ll, s_part, &props);
  (void)cs_block_excl_scan(t < BURST_CLASS_WGS ? (long long)wg_revs[t] : 0ll, s_part, &revs);
  if (threadIdx.x == 0) {
    const long long surv = classes_all & 0xffffffffll, comp = classes_all >> 32;
    counters[C_SURVIVORS] = (unsigned long long)surv;
    counters[C_COMPLETE] = (unsigned long long)comp;
    counters[C_CUTS] = (unsigned long long)cuts;
    counters[C_PROPS] = (unsigned long long)props;
    counters[C_REVS] = (unsigned long long)revs;
    const unsigned long long base = burst[B_TOP], top = base + (unsigned long long)surv;
    burst[B_SCATTER_BASE] = base;
    burst[B_TOP] = top;
    if (top > burst[B_PEAK]) burst[B_PEAK] = top;
    burst[B_CUTS] += (unsigned long long)cuts;
    burst[B_PROPS] += (unsigned long long)props;
    burst[B_REVS] += (unsigned long long)revs;
  }
}

/* copy survivor k (child surv_list[k]) into pool row new_top + k: a workgroup takes cpb (at most SB) consecutive
 * survivors and walks their cpb * n elements flat, so that small models fill the lanes too.  The number of
 * survivors is on the device; the grid is sized for the number of children. */
__global__ __launch_bounds__(SB) void cs_scatter(const cs_val *__restrict__ child_states, const int *__restrict__ surv_list,
                                                 const unsigned long long *__restrict__ counters, long long new_top, int n,
                                                 cs_val *__restrict__ pool,
                                                 const unsigned long long *__restrict__ child_forb,
                                                 unsigned long long *__restrict__ pool_forb, int fw, int cpb,
                                                 const unsigned long long *__restrict__ new_top_dev) {
  __shared__ int s_src[SB];
  if (new_top_dev != nullptr) new_top = (long long)*new_top_dev;
  const long long survivors = (long long)counters[C_SURVIVORS];
  const long long base = (long long)blockIdx.x * cpb;
  if (base >= survivors) return;
  const int here = survivors - base < cpb ? (int)(survivors - base) : cpb;
  if ((int)threadIdx.x < here) s_src[threadIdx.x] = surv_list[base + threadIdx.x];
  __syncthreads();
  const unsigned total = (unsigned)here * (unsigned)n;
  cs_val *dst = pool + (size_t)(new_top + base) * n;
  for (unsigned e = threadIdx.x; e < total; e += SB) {
    const unsigned c = e / (unsigned)n, v = e - c * (unsigned)n;
    dst[e] = child_states[(size_t)s_src[c] * n + v];
  }
  if (fw > 0) {
    const unsigned nf = (unsigned)n * (unsigned)fw, total_f = (unsigned)here * nf;
    unsigned long long *fd = pool_forb + (size_t)(new_top + base) * nf;
    for (unsigned e = threadIdx.x; e < total_f; e += SB) {
      const unsigned c = e / nf, k = e - c * nf;
      fd[e] = child_forb[(size_t)s_src[c] * nf + k];
    }
  }
}

/* nodes {-1,0,0,row}: "rebuild the forbidden sets of this state" */
__global__ void cs_fill_rebuild(csgpu_node *__restrict__ nodes, long long first_row, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  csgpu_node nd;
  nd.var = -1; nd.lo = 0; nd.hi = 0; nd.parent = (int)(first_row + i);
  nodes[i] = nd;
}

/* one wave per complete child: gather it for the root evaluation */
__global__ __launch_bounds__(SB) void cs_gather_complete(const cs_val *__restrict__ child_states,
                                                         const int *__restrict__ list, int count, int n,
                                                         cs_val *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (SB / 64) + (threadIdx.x >> 6);
  if (i >= count) return;
  const cs_val *src = child_states + (size_t)list[i] * n;
  cs_val *dst = out + (size_t)i * n;
  for (int v = lane; v < n; v += 64) dst[v] = src[v];
}

/* accept the complete children whose root evaluated to true: count, incumbent, store some.
 * One thread per complete child; one atomic per wave for the count and the incumbent.
 * stream != nullptr (ALL, ANY): every accepted child is also appended to the solution stream -- slots reserved once per
 * workgroup, at counters[C_STREAM], like the count. */
__global__ __launch_bounds__(SB) void cs_accept(const cs_val *__restrict__ complete, const int *__restrict__ truth,
                                                int count, int n, int objective, int obj_var,
                                                unsigned long long *__restrict__ counters,
                                                int32_t *__restrict__ solutions, long long max_solutions,
                                                const int *__restrict__ list /* nullable: child i is row list[i] */,
                                                int32_t *__restrict__ stream, long long stream_cap) {
  const int lane = threadIdx.x & 63;
  int i = blockIdx.x * SB + threadIdx.x;
  if (objective == CS_OBJ_ANY) {
    /* found_any (csolve.c:207-209): exactly one solution is accepted -- the first complete child,
     * in child order, whose root evaluates to true; one thread does the scan */
    if (i != 0) return;
    int first = -1;
    for (int k = 0; k < count && first < 0; k++)
      if (truth == nullptr || truth[k] == 1) first = k;
    if (first < 0 || counters[C_STORED] != 0ull) return;
    counters[C_SOLUTIONS] += 1ull;
    counters[C_STORED] = 1ull;
    long long slot = -1;
    if (stream != nullptr) {
      const unsigned long long at = counters[C_STREAM];
      slot = cs_stream_take(counters, at, 1u, stream_cap);
      if (slot >= 0) counters[C_STREAM] = at + 1ull;
    }
    for (int v = 0; v < n; v++) {
      const int32_t x = complete[(size_t)(list != nullptr ? list[first] : first) * n + v].lo;
      solutions[v] = x;
      if (slot >= 0) stream[(size_t)slot * n + v] = x;
    }
    return;
  }
  /* the count goes through LDS: one device atomic per workgroup (a word takes about 88 atomics per microsecond, and an
   * ALL iteration of queens-16 accepts 80,000 children: one atomic per wave was 14 of the kernel's 17 us) */
  __shared__ unsigned s_accepted;
  __shared__ unsigned long long s_stream0;
  if (threadIdx.x == 0) s_accepted = 0u;
  __syncthreads();
  const bool ok = i < count && (truth == nullptr || truth[i] == 1); /* truth == NULL: every complete child is a solution */
  const size_t row = ok ? (size_t)(list != nullptr ? list[i] : i) * n : 0;
  const unsigned long long mask = __ballot(ok);
  const int accepted = __popcll(mask), leader = mask != 0ull ? __builtin_ctzll(mask) : 0;
  unsigned wave_off = 0u; /* the wave's first row among the workgroup's accepted children */
  if (mask != 0ull && lane == leader) wave_off = atomicAdd(&s_accepted, (unsigned)accepted);
  __syncthreads();
  if (threadIdx.x == 0 && s_accepted != 0u) atomicAdd(&counters[C_SOLUTIONS], (unsigned long long)s_accepted);
  if (stream != nullptr) { /* uniform: the workgroup's stream rows, one device atomic */
    if (threadIdx.x == 0) s_stream0 = s_accepted != 0u ? atomicAdd(&counters[C_STREAM], (unsigned long long)s_accepted) : 0ull;
    __syncthreads();
    wave_off = (unsigned)__shfl((int)wave_off, leader);
    if (ok) {
      const unsigned long long at =
          s_stream0 + wave_off + (unsigned)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
      const long long r = cs_stream_take(counters, at, 1u, stream_cap);
      if (r >= 0)
        for (int v = 0; v < n; v++) stream[(size_t)r * n + v] = complete[row + v].lo;
    }
  }
  if (mask == 0ull) return;
  if (objective == CS_OBJ_MIN || objective == CS_OBJ_MAX) {
    int val = objective == CS_OBJ_MIN ? 0x7fffffff : (int)0x80000000;
    if (ok) val = objective == CS_OBJ_MIN ? complete[row + obj_var].lo : complete[row + obj_var].hi;
    for (int o = 32; o > 0; o >>= 1) {
      const int other = __shfl_xor(val, o);
      val = objective == CS_OBJ_MIN ? (other < val ? other : val) : (other > val ? other : val);
    }
    if (lane == leader) {
      if (objective == CS_OBJ_MIN) atomicMin((int *)&counters[C_BEST], val);
      else atomicMax((int *)&counters[C_BEST], val);
    }
  }
  long long slot0 = max_solutions;
  if (lane == leader) {
    /* which solutions are kept may vary; their count does not.  Once the store is full nobody asks for a slot */
    if (counters[C_STORED] < (unsigned long long)max_solutions)
      slot0 = (long long)atomicAdd(&counters[C_STORED], (unsigned long long)accepted);
  }
  slot0 = __shfl(slot0, leader);
  if (ok) {
    /* rank among the accepted lanes below this one: mbcnt, not a 64-bit shift by the lane number (tools/k4_fault_repro.md) */
    const long long slot = slot0 + (long long)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    if (slot < max_solutions)
      for (int v = 0; v < n; v++) solutions[(size_t)slot * n + v] = complete[row + v].lo;
  }
}

/* one wave: the first accepted complete child whose objective value equals the incumbent (stream != nullptr: appended
 * to the solution stream as well) */
__global__ void cs_pick_best(const cs_val *__restrict__ complete, const int *__restrict__ truth, int count, int n,
                             int objective, int obj_var, int best, int32_t *__restrict__ out,
                             int32_t *__restrict__ stream, long long stream_cap, unsigned long long *__restrict__ counters) {
  const int lane = threadIdx.x;
  int pick = -1;
  for (int k = 0; k < count && pick < 0; k++) {
    const cs_val o = complete[(size_t)k * n + obj_var];
    if (truth[k] == 1 && (objective == CS_OBJ_MIN ? o.lo : o.hi) == best) pick = k;
  }
  if (pick < 0) return;
  long long slot = -1;
  if (stream != nullptr) {
    const unsigned long long at = counters[C_STREAM]; /* every lane reads before lane 0 writes: one wave */
    slot = at + 1ull > counters[C_STREAM_HEAD] + (unsigned long long)stream_cap ? -1ll
                                                                               : (long long)(at % (unsigned long long)stream_cap);
    if (lane == 0) {
      if (slot >= 0) counters[C_STREAM] = at + 1ull;
      else counters[C_STREAM_ERR] = 1ull;
    }
  }
  for (int v = lane; v < n; v += 64) {
    const int32_t x = complete[(size_t)pick * n + v].lo;
    out[v] = x;
    if (slot >= 0) stream[(size_t)slot * n + v] = x;
  }
}

/* move the newest `count` rows into the hole left by taking the oldest ones */
__global__ __launch_bounds__(SB) void cs_move_rows(unsigned long long *__restrict__ pool, long long src_row,
                                                   long long dst_row, int count, int words_per_row) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (SB / 64) + (threadIdx.x >> 6);
  if (i >= count) return;
  const unsigned long long *src = pool + (size_t)(src_row + i) * words_per_row;
  unsigned long long *dst = pool + (size_t)(dst_row + i) * words_per_row;
  for (int v = lane; v < words_per_row; v += 64) dst[v] = src[v];
}

#endif
