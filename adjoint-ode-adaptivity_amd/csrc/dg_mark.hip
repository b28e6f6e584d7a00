// dg_mark.hip — marking strategies and the multi-element split of the spatial adapt loop:
// dg_plan_mark (which elements to refine, from a length-K indicator) and dg_plan_refine_marked
// (split every marked element at its midpoint in one pass).  They generalise the reference's
// one-split-per-sweep step (python/Main_finite_difference.py:336-341, matlab/MAIN.m:137-141;
// here dg_argmax + dg_plan_refine) to a set of elements per sweep.
//
// Everything ranks by ONE total order, dg_argmax(use_abs = 1)'s (`better`, dg_advec.hip): the
// key of x is the 64 bits of |x| as an unsigned integer (positive doubles order like their bit
// patterns, -0 == +0, +inf above every finite value), NaN's key is all ones (NaN ranks first,
// numpy's argmax), a larger key ranks first and equal keys rank by the lower index.
//
// The top-m set comes from an exact radix select on the key, most significant digit first:
// per-workgroup LDS histograms merged with integer atomics (order-independent, so every run
// gives the same bits; no floating-point atomic anywhere in this file), then one small
// workgroup picks the digit.  The result is the threshold key T, the count G of keys above
// it and r = m - G; the marked set is {key > T} plus the r lowest-index elements with
// key == T, which needs an exclusive scan of the "== T" flags.  That scan, and the scan of the
// marks that gives the split its offsets, is reduce-then-scan over three launches (sums per
// workgroup, one workgroup scanning the sums in a loop with a carry, apply): no inter-workgroup
// flags and no spin-waits.
#include "dg_common.h"

namespace {
using namespace dgk;

constexpr int kMarkItems = 4;                     // elements per lane
constexpr int kMarkElems = kBlock * kMarkItems;   // elements per workgroup (histogram / scan)
constexpr int kMarkGrid = 1024;                   // workgroups of the whole-array reductions
constexpr int kScanPer = 8;                       // block sums per lane of the scanning workgroup
constexpr int kScanSums = kBlock * kScanPer;      // block sums it consumes per iteration
constexpr int kDigitBits = 8;                     // one select pass settles this many key bits
constexpr int kDigits = 1 << kDigitBits;
constexpr int kPasses = 64 / kDigitBits;
constexpr int kWaves = kBlock / 64;
constexpr int kSegs = kMarkItems * kWaves;        // 64-element runs of a workgroup's range
static_assert(kDigits == kBlock, "one histogram bin per lane");
static_assert(kBlock % 64 == 0, "whole waves");

constexpr unsigned long long kKeyInf = 0x7ff0000000000000ull;
constexpr unsigned long long kKeyNaN = ~0ull;

struct MarkState {
  unsigned long long maxkey;     // key of the top-ranked entry
  unsigned long long nonfinite;  // entries that are NaN or +-inf
  unsigned long long prefix;     // the select's digits so far; after k_mark_end: T
  long long m_rem;               // ranks still to place below the prefix; after k_mark_end: r
  unsigned long long tc;         // DG_MARK_MAX_FRACTION: candidates are key >= tc
  long long total;               // dg_plan_refine_marked: the scan's total
  unsigned int hist[kPasses][kDigits];
};
static_assert(sizeof(MarkState) <= kMarkBytes, "the plan's marking buffer holds the state");

__device__ __forceinline__ unsigned long long mark_key(double x) {
  const unsigned long long b =
      static_cast<unsigned long long>(__double_as_longlong(x)) & 0x7fffffffffffffffull;
  return b > kKeyInf ? kKeyNaN : b;
}

// Element j*kBlock + lane of the workgroup's range [blockIdx.x * kMarkElems, ...): consecutive
// lanes read consecutive elements, and run s = j*kWaves + wave holds 64 consecutive elements,
// runs ascending in index.
__device__ __forceinline__ int64_t mark_elem(int j, int64_t chunk) {
  return chunk * kMarkElems + j * kBlock + threadIdx.x;
}
__device__ __forceinline__ int64_t mark_elem(int j) { return mark_elem(j, blockIdx.x); }

// Exclusive prefix count of the flags f[j] over the workgroup's range in index order:
// pre[j] = flagged elements of the range before element mark_elem(j); returns the range's count.
__device__ __forceinline__ int flag_scan(const bool (&f)[kMarkItems], int (&pre)[kMarkItems]) {
  __shared__ int seg[kSegs];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < kMarkItems; ++j) {
    const unsigned long long b = __ballot(f[j] ? 1 : 0);
    pre[j] = __popcll(b & below);
    if (lane == 0) seg[j * kWaves + wave] = __popcll(b);
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int j = 0; j < kMarkItems; ++j) {
    int before = 0;
#pragma unroll
    for (int s = 0; s < kSegs; ++s) {
      const int c = seg[s];
      if (s < j * kWaves + wave) before += c;
      if (j == 0) total += c;
    }
    pre[j] += before;
  }
  return total;
}

// Pass 0: the top-ranked key and the count of non-finite entries (integer max / add).  At most
// kMarkGrid workgroups, each over every gridDim.x-th chunk of kMarkElems elements: every
// workgroup ends in atomics on the same two words, which the L2 serialises (measured: one
// workgroup per chunk took 53 us at K = 2^22, the reads alone 5 us).
__global__ __launch_bounds__(kBlock) void k_mark_stats(const double* __restrict__ eta, int64_t K,
                                                       MarkState* __restrict__ st) {
  __shared__ unsigned long long smax;
  __shared__ unsigned int snf;
  if (threadIdx.x == 0) {
    smax = 0;
    snf = 0;
  }
  __syncthreads();
  unsigned long long mx = 0;
  unsigned int nf = 0;
  for (int64_t c = blockIdx.x; c * kMarkElems < K; c += gridDim.x) {
#pragma unroll
    for (int j = 0; j < kMarkItems; ++j) {
      const int64_t k = mark_elem(j, c);
      if (k < K) {
        const unsigned long long key = mark_key(eta[k]);
        mx = key > mx ? key : mx;
        nf += key >= kKeyInf ? 1u : 0u;
      }
    }
  }
  if (mx != 0) atomicMax(&smax, mx);
  if (nf != 0) atomicAdd(&snf, nf);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (smax != 0) atomicMax(&st->maxkey, smax);
    if (snf != 0) atomicAdd(&st->nonfinite, static_cast<unsigned long long>(snf));
  }
}

// One thread: the select's start and DG_MARK_MAX_FRACTION's candidate threshold.  With M the
// top-ranked |eta|: M finite -> candidates |eta_k| >= theta*M (one fp64 product) and > 0, i.e.
// key >= max(bits(theta*M), 1); M not finite -> exactly the non-finite entries, key >= bits(inf).
__global__ void k_mark_begin(MarkState* __restrict__ st, int strategy, double theta, long long m) {
  st->prefix = 0;
  st->m_rem = m;
  unsigned long long tc = 0;
  if (strategy == DG_MARK_MAX_FRACTION) {
    const unsigned long long M = st->maxkey;
    if (M < kKeyInf) {
      const double t = theta * __longlong_as_double(static_cast<long long>(M));
      tc = static_cast<unsigned long long>(__double_as_longlong(t));
      tc = tc < 1 ? 1 : tc;
    } else {
      tc = kKeyInf;
    }
  }
  st->tc = tc;
}

// Select pass for digit d (d = kPasses-1 first): histogram of digit d over the keys whose higher
// digits equal the prefix chosen so far.  At most kMarkGrid workgroups (as k_mark_stats: the
// merge is one atomic per non-empty bin and workgroup, and early passes have one or two bins).
__global__ __launch_bounds__(kBlock) void k_mark_hist(const double* __restrict__ eta, int64_t K,
                                                      MarkState* __restrict__ st, int d) {
  __shared__ unsigned int h[kDigits];
  h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long prefix = st->prefix;
  const int shift = d * kDigitBits;
  const int lane = threadIdx.x & 63;
  for (int64_t c = blockIdx.x; c * kMarkElems < K; c += gridDim.x) {
#pragma unroll
    for (int j = 0; j < kMarkItems; ++j) {
      const int64_t k = mark_elem(j, c);
      const unsigned long long key = k < K ? mark_key(eta[k]) : 0;
      // (a shift by 64 is undefined: the first pass has no higher digits)
      const bool match =
          k < K && (d == kPasses - 1 || ((key >> shift) >> kDigitBits) == prefix);
      const int bin = int((key >> shift) & (kDigits - 1));
      // The high digits of an indicator are nearly all equal (one exponent range): the lanes
      // that share the first matching lane's bin add their count once, the others one by one.
      const unsigned long long any = __ballot(match ? 1 : 0);
      if (any != 0) {
        const int leader = __ffsll(static_cast<long long>(any)) - 1;
        const int b0 = __shfl(bin, leader);
        const unsigned long long same = __ballot(match && bin == b0 ? 1 : 0);
        if (lane == leader) atomicAdd(&h[b0], static_cast<unsigned int>(__popcll(same)));
        if (match && bin != b0) atomicAdd(&h[bin], 1u);
      }
    }
  }
  __syncthreads();
  const unsigned int c = h[threadIdx.x];
  if (c != 0) atomicAdd(&st->hist[d][threadIdx.x], c);
}

// One workgroup, one lane per bin: the digit b with (count of bins above b) < m_rem <= (that
// count + bin b) joins the prefix, and the ranks placed above it leave m_rem.  Exactly one lane
// qualifies (1 <= m_rem <= matching keys, by induction from 1 <= m <= K).
__global__ __launch_bounds__(kBlock) void k_mark_pick(MarkState* __restrict__ st, int d) {
  __shared__ long long s[kDigits];
  const int bin = kDigits - 1 - threadIdx.x;  // lane 0 holds the highest digit
  const long long c = st->hist[d][bin];
  const long long m_rem = st->m_rem;
  const unsigned long long prefix = st->prefix;
  s[threadIdx.x] = c;
  __syncthreads();
  for (int off = 1; off < kDigits; off <<= 1) {
    const long long x = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
    __syncthreads();
    s[threadIdx.x] += x;
    __syncthreads();
  }
  const long long above = s[threadIdx.x] - c;
  if (above < m_rem && m_rem <= above + c) {
    st->prefix = (prefix << kDigitBits) | static_cast<unsigned long long>(bin);
    st->m_rem = m_rem - above;
  }
}

// One thread: the final (T, r).  mode 0: mark nothing; 1: the select's result; 2: every
// DG_MARK_MAX_FRACTION candidate.  clamp (MAX_FRACTION under a cap): the top-cap set and the
// candidates are both prefixes of the rank order, so the marked set is the shorter one: the
// select's when T >= tc, else the candidates {key > tc - 1} (tc >= 1).
__global__ void k_mark_end(MarkState* __restrict__ st, int mode, int clamp) {
  if (mode == 0) {
    st->prefix = kKeyNaN;
    st->m_rem = 0;
  } else if (mode == 2 || (clamp && st->prefix < st->tc)) {
    st->prefix = st->tc - 1;
    st->m_rem = 0;
  }
}

// Reduce: per-workgroup count of keys == T.
__global__ __launch_bounds__(kBlock) void k_mark_eqsum(const double* __restrict__ eta, int64_t K,
                                                       const MarkState* __restrict__ st,
                                                       int* __restrict__ sums) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const unsigned long long T = st->prefix;
  int c = 0;
#pragma unroll
  for (int j = 0; j < kMarkItems; ++j) {
    const int64_t k = mark_elem(j);
    if (k < K && mark_key(eta[k]) == T) ++c;
  }
  if (c != 0) atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = cnt;
}

// Reduce: per-workgroup count of nonzero marks.
__global__ __launch_bounds__(kBlock) void k_marks_sum(const uint8_t* __restrict__ marks,
                                                      int64_t K, int* __restrict__ sums) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int c = 0;
#pragma unroll
  for (int j = 0; j < kMarkItems; ++j) {
    const int64_t k = mark_elem(j);
    if (k < K && marks[k] != 0) ++c;
  }
  if (c != 0) atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = cnt;
}

// Scan: ONE workgroup turns the n per-workgroup sums into their exclusive prefix sums in place,
// kScanSums per iteration with a carry; the grand total goes to total[0] (nullable).
__global__ __launch_bounds__(kBlock) void k_scan_sums(int* __restrict__ sums, int64_t n,
                                                      long long* __restrict__ total) {
  __shared__ int s[kBlock];
  int carry = 0;
  for (int64_t base = 0; base < n; base += kScanSums) {
    const int64_t i0 = base + int64_t(threadIdx.x) * kScanPer;
    int v[kScanPer];
    int mine = 0;
#pragma unroll
    for (int q = 0; q < kScanPer; ++q) {
      v[q] = i0 + q < n ? sums[i0 + q] : 0;
      mine += v[q];
    }
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
      const int x = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += x;
      __syncthreads();
    }
    int run = carry + s[threadIdx.x] - mine;
    carry += s[kBlock - 1];
#pragma unroll
    for (int q = 0; q < kScanPer; ++q) {
      if (i0 + q < n) sums[i0 + q] = run;
      run += v[q];
    }
    __syncthreads();  // s is rewritten by the next iteration
  }
  if (threadIdx.x == 0 && total != nullptr) total[0] = carry;
}

// Apply: marks[k] = key > T, or key == T and fewer than r elements with key == T precede k.
// Also the pass's reductions per workgroup (k_mark_info finishes them): the marked count and the
// minimum marked width vx[k+1] - vx[k] (widths are positive, so their bits order as unsigned
// integers: an integer min, all ones when the workgroup marks nothing).
__global__ __launch_bounds__(kBlock) void k_mark_write(const double* __restrict__ eta, int64_t K,
                                                       const double* __restrict__ vx,
                                                       const MarkState* __restrict__ st,
                                                       const int* __restrict__ sums,
                                                       uint8_t* __restrict__ marks,
                                                       int* __restrict__ bcount,
                                                       unsigned long long* __restrict__ bminw) {
  __shared__ unsigned long long sminw;
  __shared__ int scnt;
  if (threadIdx.x == 0) {
    sminw = kKeyNaN;
    scnt = 0;
  }
  const unsigned long long T = st->prefix;
  const long long r = st->m_rem;
  unsigned long long key[kMarkItems];
  bool eq[kMarkItems];
  int pre[kMarkItems];
#pragma unroll
  for (int j = 0; j < kMarkItems; ++j) {
    const int64_t k = mark_elem(j);
    key[j] = k < K ? mark_key(eta[k]) : 0;
    eq[j] = k < K && key[j] == T;
  }
  flag_scan(eq, pre);  // (its barrier also orders the two initialisations above)
  const long long before = sums[blockIdx.x];
  int c = 0;
  unsigned long long mw = kKeyNaN;
#pragma unroll
  for (int j = 0; j < kMarkItems; ++j) {
    const int64_t k = mark_elem(j);
    if (k < K) {
      const bool m = key[j] > T || (eq[j] && before + pre[j] < r);
      marks[k] = m ? 1 : 0;
      if (m) {
        ++c;
        const unsigned long long w =
            static_cast<unsigned long long>(__double_as_longlong(vx[k + 1] - vx[k]));
        mw = w < mw ? w : mw;
      }
    }
  }
  if (c != 0) {
    atomicAdd(&scnt, c);
    atomicMin(&sminw, mw);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    bcount[blockIdx.x] = scnt;
    bminw[blockIdx.x] = sminw;
  }
}

// One workgroup sums the n per-workgroup counts, takes the min of their widths and writes the
// four result words with plain stores (info may be mapped host memory).
__global__ __launch_bounds__(kBlock) void k_mark_info(const MarkState* __restrict__ st,
                                                      const int* __restrict__ bcount,
                                                      const unsigned long long* __restrict__ bminw,
                                                      int64_t n, int64_t* __restrict__ info) {
  __shared__ unsigned long long scount, sminw;
  if (threadIdx.x == 0) {
    scount = 0;
    sminw = kKeyNaN;
  }
  __syncthreads();
  unsigned long long c = 0, mw = kKeyNaN;
  for (int64_t b = threadIdx.x; b < n; b += kBlock) {
    c += static_cast<unsigned long long>(bcount[b]);
    mw = bminw[b] < mw ? bminw[b] : mw;
  }
  if (c != 0) {
    atomicAdd(&scount, c);
    atomicMin(&sminw, mw);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    info[0] = static_cast<int64_t>(scount);
    info[1] = static_cast<int64_t>(st->nonfinite);
    info[2] = static_cast<int64_t>(scount != 0 ? sminw : kKeyInf);
    info[3] = 0;
  }
}

// Apply of the split: old element k, with o_k marked elements before it, becomes new element
// k + o_k (and k + o_k + 1 when marked: midpoint and metrics are k_refine's expressions,
// dg_advec.hip; an unmarked element's metric is copied).  sums: the scanned per-workgroup counts.
__global__ __launch_bounds__(kBlock) void k_split_marked(const uint8_t* __restrict__ marks,
                                                         int64_t K, const int* __restrict__ sums,
                                                         const double* __restrict__ vx_old,
                                                         const double* __restrict__ sc_old,
                                                         double* __restrict__ vx,
                                                         double* __restrict__ sc,
                                                         int32_t* __restrict__ parent) {
  bool f[kMarkItems];
  int pre[kMarkItems];
#pragma unroll
  for (int j = 0; j < kMarkItems; ++j) {
    const int64_t k = mark_elem(j);
    f[j] = k < K && marks[k] != 0;
  }
  flag_scan(f, pre);
  const int64_t before = sums[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kMarkItems; ++j) {
    const int64_t k = mark_elem(j);
    if (k < K) {
      const int64_t n = k + before + pre[j];
      const double xa = vx_old[k], xb = vx_old[k + 1];
      vx[n] = xa;
      if (parent != nullptr) parent[n] = int32_t(k);
      if (f[j]) {
        const double mid = 0.5 * (xa + xb);
        vx[n + 1] = mid;
        sc[n] = 2.0 / (mid - xa);
        sc[n + 1] = 2.0 / (xb - mid);
        if (parent != nullptr) parent[n + 1] = int32_t(k);
      } else {
        sc[n] = sc_old[k];
      }
      if (k == K - 1) vx[n + (f[j] ? 2 : 1)] = xb;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_parent_identity(int32_t* __restrict__ parent,
                                                            int64_t K) {
  const int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (k < K) parent[k] = int32_t(k);
}

}  // namespace

extern "C" int dg_plan_query_mark(const dg_plan* p, int64_t out[4]) {
  if (!p || !out) return fail(DG_ERR_ARG, "null argument");
  out[0] = kMarkElems;
  out[1] = kScanSums;
  out[2] = kDigitBits;
  out[3] = 0;
  return DG_OK;
}

extern "C" int dg_plan_mark(dg_plan* p, const double* eta, int strategy, double param,
                            int64_t max_marked, uint8_t* marks, int64_t* info, void* stream) {
  if (!p || !eta || !marks || !info) return fail(DG_ERR_ARG, "null argument");
  const int64_t K = p->K;
  if (const int rc = disjoint({{"eta", eta, sizeof(double) * size_t(K)},
                               {"marks", marks, size_t(K)}, {"info", info, 4 * sizeof(int64_t)}}))
    return rc;
  const int64_t cap = (max_marked < 0 || max_marked > K) ? K : max_marked;
  int mode = 0;       // k_mark_end: 0 nothing, 1 the select's set, 2 every candidate
  int64_t m = 0;      // ranks the select places
  if (strategy == DG_MARK_TOP_COUNT) {
    if (!(param >= 0.0) || param != std::floor(param))
      return fail(DG_ERR_ARG, "DG_MARK_TOP_COUNT needs an integral count m >= 0");
    m = param >= double(K) ? K : int64_t(param);
    m = m < cap ? m : cap;
    mode = m > 0 ? 1 : 0;
  } else if (strategy == DG_MARK_MAX_FRACTION) {
    if (!(param > 0.0 && param <= 1.0))
      return fail(DG_ERR_ARG, "DG_MARK_MAX_FRACTION needs theta in (0, 1]");
    // no more than K candidates exist: a cap of K or more never truncates
    m = cap;
    mode = cap >= K ? 2 : (cap > 0 ? 1 : 0);
  } else {
    return fail(DG_ERR_ARG, "unknown marking strategy");
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MarkState* ms = static_cast<MarkState*>(p->d_mark);
  const unsigned grid = grid_for(K, kMarkElems);
  const unsigned rgrid = grid < unsigned(kMarkGrid) ? grid : unsigned(kMarkGrid);
  // per workgroup, in the plan's second scratch field (16 B each; the field has 16 B per element
  // or more): the minimum marked width, the "== T" count and its scan, the marked count
  unsigned long long* bminw = reinterpret_cast<unsigned long long*>(p->d_scratch2);
  int* sums = reinterpret_cast<int*>(bminw + grid);
  int* bcount = sums + grid;
  HIP_TRY(hipMemsetAsync(ms, 0, sizeof(MarkState), st));
  hipLaunchKernelGGL(k_mark_stats, dim3(rgrid), dim3(kBlock), 0, st, eta, K, ms);
  hipLaunchKernelGGL(k_mark_begin, dim3(1), dim3(1), 0, st, ms, strategy, param,
                     static_cast<long long>(m));
  if (mode == 1) {
    for (int d = kPasses - 1; d >= 0; --d) {
      hipLaunchKernelGGL(k_mark_hist, dim3(rgrid), dim3(kBlock), 0, st, eta, K, ms, d);
      hipLaunchKernelGGL(k_mark_pick, dim3(1), dim3(kBlock), 0, st, ms, d);
    }
  }
  hipLaunchKernelGGL(k_mark_end, dim3(1), dim3(1), 0, st, ms, mode,
                     strategy == DG_MARK_MAX_FRACTION ? 1 : 0);
  hipLaunchKernelGGL(k_mark_eqsum, dim3(grid), dim3(kBlock), 0, st, eta, K, ms, sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kBlock), 0, st, sums, int64_t(grid),
                     static_cast<long long*>(nullptr));
  hipLaunchKernelGGL(k_mark_write, dim3(grid), dim3(kBlock), 0, st, eta, K, p->d_VX, ms, sums,
                     marks, bcount, bminw);
  hipLaunchKernelGGL(k_mark_info, dim3(1), dim3(kBlock), 0, st, ms, bcount, bminw,
                     int64_t(grid), info);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}

extern "C" int dg_plan_refine_marked(dg_plan* p, const uint8_t* marks, int32_t* parent,
                                     int64_t* n_split, void* stream) {
  if (!p || !marks) return fail(DG_ERR_ARG, "null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MarkState* ms = static_cast<MarkState*>(p->d_mark);
  int* sums = reinterpret_cast<int*>(p->d_scratch2);
  const int64_t K = p->K;
  // parent holds K + splits entries: at least K, checked before anything is enqueued, and its
  // true extent again below once the scan has counted the splits (before parent or the mesh is
  // written; the scan only reads marks and writes plan scratch)
  if (const int rc = disjoint({{"marks", marks, size_t(K)},
                               {"parent", parent, sizeof(int32_t) * size_t(K)}}))
    return rc;
  const unsigned grid = grid_for(K, kMarkElems);
  hipLaunchKernelGGL(k_marks_sum, dim3(grid), dim3(kBlock), 0, st, marks, K, sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kBlock), 0, st, sums, int64_t(grid), &ms->total);
  HIP_TRY(hipGetLastError());
  long long total = 0;
  HIP_TRY(hipMemcpyAsync(&total, &ms->total, sizeof(total), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (total < 0 || total > K) return fail(DG_ERR_HIP, "marks scan returned an impossible total");
  if (K + total > p->K_cap)
    return fail(DG_ERR_ARG, "marked splits exceed the plan's capacity: call dg_plan_reserve "
                            "first, or mark with max_marked = capacity - K");
  if (const int rc = disjoint({{"marks", marks, size_t(K)},
                               {"parent", parent, sizeof(int32_t) * size_t(K + total)}}))
    return rc;
  if (total == 0) {
    // nothing to split: the mesh (and `uniform`) stay as they are; parent is the identity
    if (parent != nullptr) {
      hipLaunchKernelGGL(k_parent_identity, dim3(grid_for(K, kBlock)), dim3(kBlock), 0, st, parent,
                         K);
      HIP_TRY(hipGetLastError());
    }
    if (n_split) *n_split = 0;
    return DG_OK;
  }
  // The old mesh goes to scratch first (the split shifts it in place), as dg_plan_refine.
  // total >= 1 and K + total <= K_cap leave room for its 2K + 1 doubles.
  double* vx_old = p->d_scratch;
  double* sc_old = p->d_scratch + (K + 1);
  HIP_TRY(hipMemcpyAsync(vx_old, p->d_VX, sizeof(double) * (K + 1), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(sc_old, p->d_scale, sizeof(double) * K, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_split_marked, dim3(grid), dim3(kBlock), 0, st, marks, K, sums, vx_old,
                     sc_old, p->d_VX, p->d_scale, parent);
  HIP_TRY(hipGetLastError());
  p->K += total;
  p->ktot = p->K * p->batch;
  p->uniform = false;  // every element now uses its own 2/h_k
  if (n_split) *n_split = total;
  return DG_OK;
}
