// dg_transfer.hip — carrying a nodal field across a one-level refinement of the mesh:
// dg_field_to_children (every new element from its parent) and dg_field_from_children (every
// old element from its one or two children).  The refinement is the midpoint split of
// python/Main_finite_difference.py:336-341 / matlab/MAIN.m:137-141 as dg_plan_refine and
// dg_plan_refine_marked perform it; the field transfer is the interpU role of
// python/factory.py:281-286.
//
// A split element's children have their nodes at the parent's reference coordinates (r - 1)/2
// (left) and (r + 1)/2 (right).  The LGL nodes are symmetric, so with J the node reversal the
// right child's matrix is J A J for the left child's A: one Np x Np matrix, handed over by the
// caller, serves both kernels and every operator built on them (prolongation A = PL, its
// transpose A = PL^T, the L2 projection A = RL).  A right child therefore runs the left child's
// arithmetic on reversed nodes, and an unsplit element takes its values through a select, so a
// wave runs one instruction stream whatever its lanes' roles and A stays wave-uniform (it is
// read from the kernel-argument segment).
//
// Both kernels are streaming kernels, one lane per NEW element.  The new field's side of a
// workgroup is the contiguous run of its 256 elements and passes through an LDS image, so that
// global memory is accessed 16 bytes per lane, lane-consecutive.  The old field's side is
// contiguous too: parent is nondecreasing in steps of 0 or 1 from 0 to k_old - 1, so the old
// element b * k_old + parent[n] never steps by more than one from lane to lane (also from one
// trajectory's last element to the next one's first) and a workgroup's lanes touch at most 256
// consecutive old elements, starting at lane 0's.  k_from_children stores them through the
// image as well (a lane whose old element lies outside that window, an ill-formed map, stores
// directly); k_to_children reads them per lane, which measured faster than an image of them
// (DESIGN.md §5).  No atomics: every output double is written by exactly one lane, so equal
// inputs give equal bits.
#include "dg_common.h"

namespace {
using namespace dgk;

template <int NP> struct TransferArgs {
  double A[NP * NP];  // the left child's matrix, row-major
  int64_t total;      // batch * K_new
  int64_t total_old;  // batch * k_old
  int32_t k_new;
  int32_t k_old;
  int32_t vec_in;     // in / out are 16-byte aligned: 16-byte accesses
  int32_t vec_out;
};

// Rows of the LDS image are an odd number of doubles apart: lanes accessing their own row do
// not meet in one bank at even Np.
template <int NP> constexpr int kRow = NP | 1;
template <int NP> constexpr int kImage = (kBlock + 1) * kRow<NP>;

// Image position of double i of the run (row i / Np).
template <int NP> __device__ __forceinline__ int img_pos(int i) {
  const int el = i / NP;
  return el * kRow<NP> + (i - el * NP);
}

// img <- g[d0, d0 + cnt): lane-consecutive 16-byte loads from the even double at or below d0
// (vec: g is 16-byte aligned), 8-byte loads otherwise and at the run's odd ends.
template <int NP>
__device__ __forceinline__ void image_load(const double* __restrict__ g, int64_t d0, int cnt,
                                           double* __restrict__ img, bool vec) {
  const int off = int(d0 & 1);
  const double* __restrict__ g0 = g + (d0 - off);
  const int npairs = (cnt + off + 1) >> 1;
  for (int v = threadIdx.x; v < npairs; v += kBlock) {
    const int i0 = 2 * v - off, i1 = i0 + 1;
    const bool in0 = i0 >= 0, in1 = i1 < cnt;
    if (vec && in0 && in1) {
      const double2 t = *reinterpret_cast<const double2*>(g0 + 2 * v);
      img[img_pos<NP>(i0)] = t.x;
      img[img_pos<NP>(i1)] = t.y;
    } else {
      if (in0) img[img_pos<NP>(i0)] = g0[2 * v];
      if (in1) img[img_pos<NP>(i1)] = g0[2 * v + 1];
    }
  }
}

// g[d0, d0 + cnt) <- img, only the rows whose flag is set; accesses as image_load.
template <int NP>
__device__ __forceinline__ void image_store(double* __restrict__ g, int64_t d0, int cnt,
                                            const double* __restrict__ img,
                                            const uint8_t* __restrict__ flags, bool vec) {
  const int off = int(d0 & 1);
  double* __restrict__ g0 = g + (d0 - off);
  const int npairs = (cnt + off + 1) >> 1;
  for (int v = threadIdx.x; v < npairs; v += kBlock) {
    const int i0 = 2 * v - off, i1 = i0 + 1;
    const bool f0 = i0 >= 0 && flags[i0 / NP] != 0;
    const bool f1 = i1 < cnt && flags[i1 / NP] != 0;
    if (vec && f0 && f1) {
      double2 t;
      t.x = img[img_pos<NP>(i0)];
      t.y = img[img_pos<NP>(i1)];
      *reinterpret_cast<double2*>(g0 + 2 * v) = t;
    } else {
      if (f0) g0[2 * v] = img[img_pos<NP>(i0)];
      if (f1) g0[2 * v + 1] = img[img_pos<NP>(i1)];
    }
  }
}

// What new element n is.  parent[n - 1] and parent[n + 1] are read only inside [0, K_new);
// `ok` is false for a parent outside [0, k_old): such a lane neither reads nor writes a field.
struct Role {
  int32_t p;
  bool ok, left, right;
};

__device__ __forceinline__ Role role_of(const int32_t* __restrict__ parent, int32_t n,
                                        int32_t k_new, int32_t k_old) {
  Role r;
  r.p = parent[n];
  r.ok = r.p >= 0 && r.p < k_old;
  r.right = n > 0 && parent[n - 1] == r.p;
  r.left = !r.right && n + 1 < k_new && parent[n + 1] == r.p;
  return r;
}

// The old element of the workgroup's first lane: the start of its window of kBlock old
// elements (workgroup-uniform; an out-of-range parent counts as 0).
__device__ __forceinline__ int64_t window_base(const int32_t* __restrict__ parent, int64_t e0,
                                               int32_t k_new, int32_t k_old) {
  // total < 2^31 (checked at plan creation): 32-bit division
  const uint32_t b0 = uint32_t(e0) / uint32_t(k_new);
  const int32_t p0 = parent[uint32_t(e0) - b0 * uint32_t(k_new)];
  return int64_t(b0) * k_old + (p0 >= 0 && p0 < k_old ? p0 : 0);
}

// out_new[e] = in_old[parent] (unsplit, a copy of the bits), A in (left child) or J A J in
// (right child).
template <int NP>
__global__ __launch_bounds__(kBlock) void k_to_children(const double* __restrict__ in,
                                                        double* __restrict__ out,
                                                        const int32_t* __restrict__ parent,
                                                        TransferArgs<NP> a) {
  constexpr int SP = kRow<NP>;
  __shared__ double img[kImage<NP>];
  __shared__ uint8_t okf[kBlock];
  const int64_t e0 = int64_t(blockIdx.x) * kBlock;
  const int64_t e = e0 + threadIdx.x;
  bool ok = false;
  if (e < a.total) {
    // total < 2^31 (checked at plan creation): 32-bit division
    const uint32_t b = uint32_t(e) / uint32_t(a.k_new);
    const int32_t n = int32_t(uint32_t(e) - b * uint32_t(a.k_new));
    const Role r = role_of(parent, n, a.k_new, a.k_old);
    ok = r.ok;
    if (ok) {
      // the parent's run of Np doubles, per lane: neighbouring lanes' runs are neighbours or
      // the same run
      const double* __restrict__ row = in + (int64_t(b) * a.k_old + r.p) * NP;
      const bool split = r.left || r.right;
      double v[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) v[j] = row[r.right ? NP - 1 - j : j];
      double* __restrict__ o = img + threadIdx.x * SP;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        double t = a.A[i * NP] * v[0];
#pragma unroll
        for (int j = 1; j < NP; ++j) t = fma(a.A[i * NP + j], v[j], t);
        o[r.right ? NP - 1 - i : i] = split ? t : v[i];
      }
    }
  }
  okf[threadIdx.x] = ok ? 1 : 0;
  __syncthreads();
  const int64_t rem = a.total - e0;
  image_store<NP>(out, e0 * NP, int(rem < kBlock ? rem : kBlock) * NP, img, okf, a.vec_out != 0);
}

// out_old[parent] = in_new[e] (unsplit, a copy of the bits) or A in_new[e] + J A J in_new[e + 1]
// (e the left child); a right child's lane writes nothing.
template <int NP>
__global__ __launch_bounds__(kBlock) void k_from_children(const double* __restrict__ in,
                                                          double* __restrict__ out,
                                                          const int32_t* __restrict__ parent,
                                                          TransferArgs<NP> a) {
  constexpr int SP = kRow<NP>;
  __shared__ double img[kImage<NP>];  // kBlock rows + the last lane's right sibling
  __shared__ uint8_t okf[kBlock];
  const int64_t e0 = int64_t(blockIdx.x) * kBlock;
  const int64_t e = e0 + threadIdx.x;
  const int64_t rem = a.total - e0;
  image_load<NP>(in, e0 * NP, int(rem < kBlock + 1 ? rem : kBlock + 1) * NP, img,
                 a.vec_in != 0);
  okf[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = window_base(parent, e0, a.k_new, a.k_old);
  bool writer = false;
  int64_t g = 0;
  double res[NP];
  if (e < a.total) {
    const uint32_t b = uint32_t(e) / uint32_t(a.k_new);
    const int32_t n = int32_t(uint32_t(e) - b * uint32_t(a.k_new));
    const Role r = role_of(parent, n, a.k_new, a.k_old);
    writer = r.ok && !r.right;
    if (writer) {
      g = int64_t(b) * a.k_old + r.p;
      // (a left child's sibling is element e + 1 of the same trajectory: n + 1 < K_new; the
      // other lanes read a row they do not use)
      const double* __restrict__ mine = img + threadIdx.x * SP;
      const double* __restrict__ next = mine + SP;
      double v[NP], w[NP], t[NP], s[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        v[j] = mine[j];
        w[j] = next[NP - 1 - j];
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        double ti = a.A[i * NP] * v[0], si = a.A[i * NP] * w[0];
#pragma unroll
        for (int j = 1; j < NP; ++j) {
          ti = fma(a.A[i * NP + j], v[j], ti);
          si = fma(a.A[i * NP + j], w[j], si);
        }
        t[i] = ti;
        s[i] = si;
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) res[i] = r.left ? t[i] + s[NP - 1 - i] : v[i];
    }
  }
  __syncthreads();  // the new field's image is read: the old field's replaces it
  if (writer) {
    const int64_t slot = g - base;
    if (slot >= 0 && slot < kBlock) {
      double* __restrict__ o = img + int(slot) * SP;
#pragma unroll
      for (int i = 0; i < NP; ++i) o[i] = res[i];
      okf[slot] = 1;
    } else {
      double* __restrict__ o = out + g * NP;
#pragma unroll
      for (int i = 0; i < NP; ++i) o[i] = res[i];
    }
  }
  __syncthreads();
  const int64_t left_old = a.total_old - base;
  image_store<NP>(out, base * NP, int(left_old < kBlock ? left_old : kBlock) * NP, img, okf,
                  a.vec_out != 0);
}

template <bool TO>
int transfer(const dg_plan* p, const int32_t* parent, int64_t k_old, const double* A,
             const double* in, double* out, void* stream) {
  if (!p || !parent || !A || !in || !out) return fail(DG_ERR_ARG, "null argument");
  const int64_t K = p->K;
  if (k_old < 1 || k_old > K || K > 2 * k_old)
    return fail(DG_ERR_ARG, "k_old must satisfy 1 <= k_old <= K <= 2 k_old (one level of "
                            "midpoint splits)");
  const size_t n_old = size_t(p->batch) * size_t(k_old) * size_t(p->NP) * sizeof(double);
  const size_t n_new = size_t(p->ktot) * size_t(p->NP) * sizeof(double);
  if (const int rc = disjoint({{"parent", parent, sizeof(int32_t) * size_t(K)},
                               {"in", in, TO ? n_old : n_new}, {"out", out, TO ? n_new : n_old}}))
    return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return dispatch_np(p->NP, [&](auto np) -> int {
    constexpr int NP = np;
    TransferArgs<NP> a;
    for (int i = 0; i < NP * NP; ++i) a.A[i] = A[i];
    a.total = p->ktot;
    a.total_old = p->batch * k_old;
    a.k_new = int32_t(K);
    a.k_old = int32_t(k_old);
    a.vec_in = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    a.vec_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    static_assert(sizeof(a) <= kKernargMax, "the matrix travels in the kernel arguments");
    if (TO)
      hipLaunchKernelGGL((k_to_children<NP>), dim3(grid_for(p->ktot, kBlock)), dim3(kBlock), 0,
                         st, in, out, parent, a);
    else
      hipLaunchKernelGGL((k_from_children<NP>), dim3(grid_for(p->ktot, kBlock)), dim3(kBlock),
                         0, st, in, out, parent, a);
    HIP_TRY(hipGetLastError());
    return DG_OK;
  });
}

}  // namespace

extern "C" int dg_field_to_children(const dg_plan* plan, const int32_t* parent, int64_t k_old,
                                    const double* A, const double* in_old, double* out_new,
                                    void* stream) {
  return transfer<true>(plan, parent, k_old, A, in_old, out_new, stream);
}

extern "C" int dg_field_from_children(const dg_plan* plan, const int32_t* parent, int64_t k_old,
                                      const double* A, const double* in_new, double* out_old,
                                      void* stream) {
  return transfer<false>(plan, parent, k_old, A, in_new, out_old, stream);
}
