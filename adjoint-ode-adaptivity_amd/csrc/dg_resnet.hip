// dg_resnet.hip — the ResNet-as-ODE ensemble loop of python/Main_width_ref.py with scalar
// state (the ResNet half): layer l is ResBlockSimple (models.py:60-64),
//   Phi_l(u, dt) = u + dt * sum_f W2_l[f] * relu(W1_l[f] * (u - b_l[f])),
// one ensemble member (initial condition u0[ic], label target[ic]) per lane.
//
// dg_resnet_adapt_sweep: forwardSolve (:48-68) on the coarse mesh, adjointSolve (:77-105) on
// the ref_factor-refined mesh and errorIndicator (:126-139) in one launch.  forwardFn reads
// only u[-1] (:44-45), so sumTerm(i, j) (:87-97) vanishes unless i = j - 1 and the O(n^2)
// double loop (:99-104) is the backward recursion v_{n-1} = v_n * dPhi/du(u_{n-1}); dJdU is
// nonzero at the last node only (outFnl, :71-73), where it is sign(u - target).
// The fine solution is the np.interp of the coarse one (refineSolution, :117-122), evaluated
// on the fly (dg_interp.h).
//
// dg_resnet_loss_grad: lossFn (:142-145) per member and the mean over members of the loss
// and of its gradient with respect to every b, W1, W2 (trainStep, :164-169), by
// backpropagation; the member sums run in a fixed order (no floating-point atomics).
//
// Layouts: parameters as three packed arrays bias / w1 / w2 [P], layer l at
// [off[l], off[l+1]); U[n*n_ics + ic] (coarse nodes), V[n*n_ics + ic] (fine nodes, optional),
// err_steps[ic*L + i] (layers contiguous per member, for dg_sum_rows); grad [3][P] in the
// order bias, w1, w2.
//
// The parameters are uniform across a wave: they are read through the constant address
// space, i.e. by scalar loads through the scalar cache into SGPRs, which feed the fp64 VALU
// instructions directly (no vector load, no LDS traffic, no VGPRs for them).  No kernel
// writes them.
#include "dg_common.h"
#include "dg_interp.h"

namespace {
using namespace dgk;

constexpr int kRnBlock = 256;   // members per workgroup (sweep, gradient pass A)
constexpr int kRnChunk = 256;   // members per partial sum of the gradient (pass B)
constexpr int kRnLanesB = 128;  // lanes (neurons in flight) of a pass-B workgroup
constexpr int kMaxRf = 16;
static_assert(kRnChunk == kRnBlock, "pass A's loss partials and pass B's chunks coincide");

// Layer offsets, passed by value: uniform reads from the kernel-argument segment.
struct Layers {
  int32_t off[DG_RESNET_MAX_LAYERS + 1];
};
static_assert(sizeof(Layers) + 256 <= kKernargMax, "the offsets travel as kernel arguments");

using kdouble = const DG_KAS double*;

// sum_f W2[f] relu(z_f), z_f = W1[f] (u - b[f])   (models.py:60-64)
__device__ __forceinline__ double layer_sum(kdouble b, kdouble w1, kdouble w2, int f0, int f1,
                                            double u) {
  double s = 0.0;
#pragma unroll 4
  for (int f = f0; f < f1; ++f) {
    const double z = w1[f] * (u - b[f]);
    s = fma(w2[f], fmax(z, 0.0), s);
  }
  return s;
}

// The same sum and d/du of it, sum_f W2[f] W1[f] [z_f > 0] (relu'(0) = 0 as in jax), sharing
// z_f: with g = [z > 0] W2 the two terms are g z and g W1.
__device__ __forceinline__ void layer_sum_deriv(kdouble b, kdouble w1, kdouble w2, int f0, int f1,
                                                double u, double& s, double& d) {
  s = 0.0;
  d = 0.0;
#pragma unroll 4
  for (int f = f0; f < f1; ++f) {
    const double a = w1[f], w = w2[f];  // loaded unconditionally: one wide scalar load
    const double z = a * (u - b[f]);
    const double g = z > 0.0 ? w : 0.0;
    s = fma(g, z, s);
    d = fma(g, a, d);
  }
}

__global__ __launch_bounds__(kRnBlock) void k_resnet_sweep(
    const double* __restrict__ bias, const double* __restrict__ w1, const double* __restrict__ w2,
    const double* __restrict__ dt_n, const double* __restrict__ tc, const double* __restrict__ tf,
    const int32_t* __restrict__ code, const double* __restrict__ u0,
    const double* __restrict__ target, double* __restrict__ U, double* __restrict__ V,
    double* __restrict__ err_steps, int64_t n_ics, int n_layers, int rf, Layers lay) {
  const int64_t ic = int64_t(blockIdx.x) * kRnBlock + threadIdx.x;
  if (ic >= n_ics) return;
  kdouble kb = (kdouble)bias, k1 = (kdouble)w1, k2 = (kdouble)w2;
  // forwardSolve: u_{l+1} = Phi_l(u_l, dt_l)
  double u = u0[ic];
  U[ic] = u;
  for (int l = 0; l < n_layers; ++l) {
    u = fma(dt_n[l], layer_sum(kb, k1, k2, lay.off[l], lay.off[l + 1], u), u);
    U[int64_t(l + 1) * n_ics + ic] = u;
  }
  // Backward over the fine grid.  v_nf = sign(u_fine[nf] - target) (grad of outFnl);
  // res_n = u_fine[n] - Phi(u_fine[n-1], dt_fine[n-1]) with the parameters of layer
  // (n-1)//rf;  v_{n-1} = v_n (1 + dt_fine[n-1] dsum(u_fine[n-1])).  Layer m's window is the
  // fine steps n = m rf + 1 .. (m+1) rf (:136-138): res_n v_n is summed over the whole
  // window, here from its last step down, and the absolute value is taken of the sum.
  const int nf = n_layers * rf;
  double un = fine_u(code[nf], tf[nf], tc, U, n_ics, ic);
  const double diff = un - target[ic];
  double v = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0);
  if (V) V[int64_t(nf) * n_ics + ic] = v;
  double* __restrict__ erow = err_steps + ic * n_layers;
  for (int m = n_layers - 1; m >= 0; --m) {
    const double dtp = dt_n[m] / double(rf);  // refineTime, :108-114
    const int f0 = lay.off[m], f1 = lay.off[m + 1];
    double acc = 0.0;
    for (int p = rf - 1; p >= 0; --p) {
      const int n = m * rf + 1 + p;  // fine step n: nodes n-1 -> n
      const double up = fine_u(code[n - 1], tf[n - 1], tc, U, n_ics, ic);
      double s, d;
      layer_sum_deriv(kb, k1, k2, f0, f1, up, s, d);
      const double res = un - fma(dtp, s, up);
      acc = fma(res, v, acc);
      v = v * fma(dtp, d, 1.0);
      if (V) V[int64_t(n - 1) * n_ics + ic] = v;
      un = up;
    }
    erow[m] = fabs(acc);
  }
}

// Gradient pass A, one lane per member: the forward states u_l (l < L) into Us[l*n_ics+ic],
// the loss (u_L - target)^2, then backwards q_l = lambda_{l+1} dt_l into Qs[l*n_ics+ic]
// with lambda_L = 2 (u_L - target), lambda_l = lambda_{l+1} dPhi_l/du(u_l).  The workgroup's
// losses are summed by a stride-halving tree (128, 64, .., 1) into loss_part[block].
__global__ __launch_bounds__(kRnBlock) void k_resnet_grad_a(
    const double* __restrict__ bias, const double* __restrict__ w1, const double* __restrict__ w2,
    const double* __restrict__ dt_n, const double* __restrict__ u0,
    const double* __restrict__ target, double* __restrict__ Us, double* __restrict__ Qs,
    double* __restrict__ loss_ic, double* __restrict__ loss_part, int64_t n_ics, int n_layers,
    Layers lay) {
  __shared__ double red[kRnBlock];
  const int64_t ic = int64_t(blockIdx.x) * kRnBlock + threadIdx.x;
  kdouble kb = (kdouble)bias, k1 = (kdouble)w1, k2 = (kdouble)w2;
  double loss = 0.0;
  if (ic < n_ics) {
    double u = u0[ic];
    for (int l = 0; l < n_layers; ++l) {
      Us[int64_t(l) * n_ics + ic] = u;
      u = fma(dt_n[l], layer_sum(kb, k1, k2, lay.off[l], lay.off[l + 1], u), u);
    }
    const double r = u - target[ic];
    loss = r * r;
    if (loss_ic) loss_ic[ic] = loss;
    double lam = 2.0 * r;
    for (int l = n_layers - 1; l >= 0; --l) {
      const double dt = dt_n[l];
      Qs[int64_t(l) * n_ics + ic] = lam * dt;
      if (l > 0) {
        double s, d;
        layer_sum_deriv(kb, k1, k2, lay.off[l], lay.off[l + 1], Us[int64_t(l) * n_ics + ic], s, d);
        lam = lam * fma(dt, d, 1.0);
      }
    }
  }
  red[threadIdx.x] = loss;
  __syncthreads();
#pragma unroll
  for (int h = kRnBlock / 2; h >= 1; h >>= 1) {
    if (int(threadIdx.x) < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_part[blockIdx.x] = red[0];
}

// Gradient pass B, workgroup (chunk c, layer l), one lane per neuron f of the layer (lanes
// stride over wider layers): the chunk's (u_l, q_l) pairs are staged in LDS once, then every
// lane walks the chunk's members in ascending order (all lanes read the same LDS address: a
// broadcast) and accumulates its three parameters privately.  With t = u - b, z = W1 t,
// m = [z > 0] q:  dW2 += m z,  dW1 += W2 m t,  db += -W2 W1 m  (the W2 factors applied once,
// after the walk).  part[(c*3 + k)*P + off[l] + f], k = 0 bias, 1 w1, 2 w2.
__global__ __launch_bounds__(kRnLanesB) void k_resnet_grad_b(
    const double* __restrict__ bias, const double* __restrict__ w1, const double* __restrict__ w2,
    const double* __restrict__ Us, const double* __restrict__ Qs, double* __restrict__ part,
    int64_t n_ics, int64_t P, Layers lay) {
  __shared__ double2 uq[kRnChunk];
  const int l = blockIdx.y;
  const int64_t c = blockIdx.x, i0 = c * kRnChunk;
  const int cnt = int(n_ics - i0 < kRnChunk ? n_ics - i0 : kRnChunk);
  for (int i = threadIdx.x; i < cnt; i += kRnLanesB)
    uq[i] = make_double2(Us[int64_t(l) * n_ics + i0 + i], Qs[int64_t(l) * n_ics + i0 + i]);
  __syncthreads();
  const int f0 = lay.off[l], f1 = lay.off[l + 1];
  for (int f = f0 + int(threadIdx.x); f < f1; f += kRnLanesB) {
    const double b = bias[f], a = w1[f], w = w2[f];
    double gb = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll 4
    for (int i = 0; i < cnt; ++i) {
      const double2 e = uq[i];
      const double t = e.x - b, z = a * t;
      const double m = z > 0.0 ? e.y : 0.0;
      g2 = fma(m, z, g2);
      g1 = fma(m, t, g1);
      gb += m;
    }
    double* __restrict__ o = part + c * 3 * P + f;
    o[0] = -(w * a) * gb;
    o[P] = w * g1;
    o[2 * P] = g2;
  }
}

// Gradient pass C, one lane per gradient entry j < 3P: the chunk partials in ascending chunk
// order, then one division by n_ics; lane 3P does the same for the loss partials.  The loads
// of kCBatch chunks are issued together (their latency, not the additions, bounds this pass);
// the additions stay in ascending order.
constexpr int kCBlock = 64, kCBatch = 16;
__global__ __launch_bounds__(kCBlock) void k_resnet_grad_c(
    const double* __restrict__ part, const double* __restrict__ loss_part, int64_t n_chunks,
    int64_t P3, double n, double* __restrict__ grad, double* __restrict__ loss_mean) {
  const int64_t j = int64_t(blockIdx.x) * kCBlock + threadIdx.x;
  if (j > P3) return;
  const double* __restrict__ src = j < P3 ? part + j : loss_part;
  const int64_t ld = j < P3 ? P3 : 1;
  double acc = 0.0;
  int64_t c = 0;
  for (; c + kCBatch <= n_chunks; c += kCBatch) {
    double t[kCBatch];
#pragma unroll
    for (int i = 0; i < kCBatch; ++i) t[i] = src[(c + i) * ld];
#pragma unroll
    for (int i = 0; i < kCBatch; ++i) acc += t[i];
  }
  for (; c < n_chunks; ++c) acc += src[c * ld];
  if (j < P3) grad[j] = acc / n;
  else *loss_mean = acc / n;
}

int check_layers(int n_layers, const int32_t* offsets, Layers* lay) {
  if (!offsets) return fail(DG_ERR_ARG, "null argument");
  if (n_layers < 1) return fail(DG_ERR_ARG, "a net needs at least one layer");
  if (n_layers > DG_RESNET_MAX_LAYERS)
    return fail(DG_ERR_ARG, "more than DG_RESNET_MAX_LAYERS layers are not supported");
  if (offsets[0] != 0) return fail(DG_ERR_ARG, "offsets[0] must be 0");
  for (int l = 0; l < n_layers; ++l)
    if (offsets[l + 1] <= offsets[l]) return fail(DG_ERR_ARG, "a layer has no neurons");
  std::memset(lay, 0, sizeof(Layers));
  std::memcpy(lay->off, offsets, sizeof(int32_t) * size_t(n_layers + 1));
  return DG_OK;
}

// Scratch of dg_resnet_loss_grad in doubles: Us, Qs [L][n_ics], loss partials [chunks],
// gradient partials [chunks][3][P].
struct GradScratch {
  int64_t chunks, us, qs, loss_part, part, total;
};
GradScratch grad_scratch(int n_layers, int64_t P, int64_t n_ics) {
  GradScratch g;
  g.chunks = (n_ics + kRnChunk - 1) / kRnChunk;
  g.us = 0;
  g.qs = g.us + int64_t(n_layers) * n_ics;
  g.loss_part = g.qs + int64_t(n_layers) * n_ics;
  g.part = g.loss_part + g.chunks;
  g.total = g.part + g.chunks * 3 * P;
  return g;
}

}  // namespace

extern "C" {

int dg_resnet_adapt_sweep(int n_layers, int ref_factor, const int32_t* offsets,
                          const double* bias, const double* w1, const double* w2,
                          const double* dt_n, const double* t_coarse, const double* t_fine,
                          const int32_t* interp_code, const double* u0, const double* target,
                          int64_t n_ics, double* U, double* V, double* err_steps, void* stream) {
  if (!bias || !w1 || !w2 || !dt_n || !t_coarse || !t_fine || !interp_code || !u0 || !target ||
      !U || !err_steps)
    return fail(DG_ERR_ARG, "null argument");
  Layers lay;
  if (int rc = check_layers(n_layers, offsets, &lay)) return rc;
  if (ref_factor < 2 || n_ics < 1) return fail(DG_ERR_ARG, "bad sizes");
  if (ref_factor > kMaxRf) return fail(DG_ERR_ARG, "ref_factor > 16 is not supported");
  if ((n_ics + kRnBlock - 1) / kRnBlock > INT32_MAX) return fail(DG_ERR_ARG, "too many members");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_resnet_sweep, dim3(grid_for(n_ics, kRnBlock)), dim3(kRnBlock), 0, st, bias,
                     w1, w2, dt_n, t_coarse, t_fine, interp_code, u0, target, U, V, err_steps,
                     n_ics, n_layers, ref_factor, lay);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}

int dg_resnet_grad_scratch(int n_layers, const int32_t* offsets, int64_t n_ics, int64_t* bytes) {
  if (!bytes) return fail(DG_ERR_ARG, "null argument");
  Layers lay;
  if (int rc = check_layers(n_layers, offsets, &lay)) return rc;
  if (n_ics < 1) return fail(DG_ERR_ARG, "bad sizes");
  *bytes = grad_scratch(n_layers, lay.off[n_layers], n_ics).total * int64_t(sizeof(double));
  return DG_OK;
}

int dg_resnet_loss_grad(int n_layers, const int32_t* offsets, const double* bias,
                        const double* w1, const double* w2, const double* dt_n, const double* u0,
                        const double* target, int64_t n_ics, double* loss_ic, double* loss_mean,
                        double* grad, void* scratch, int64_t scratch_bytes, void* stream) {
  if (!bias || !w1 || !w2 || !dt_n || !u0 || !target || !loss_mean || !grad || !scratch)
    return fail(DG_ERR_ARG, "null argument");
  Layers lay;
  if (int rc = check_layers(n_layers, offsets, &lay)) return rc;
  if (n_ics < 1) return fail(DG_ERR_ARG, "bad sizes");
  const int64_t P = lay.off[n_layers];
  const GradScratch g = grad_scratch(n_layers, P, n_ics);
  if (g.chunks > INT32_MAX) return fail(DG_ERR_ARG, "too many members");
  if (scratch_bytes < g.total * int64_t(sizeof(double)))
    return fail(DG_ERR_ARG, "scratch is smaller than dg_resnet_grad_scratch reports");
  if (reinterpret_cast<uintptr_t>(scratch) % 16) return fail(DG_ERR_ARG, "scratch is misaligned");
  double* s = static_cast<double*>(scratch);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_resnet_grad_a, dim3(unsigned(g.chunks)), dim3(kRnBlock), 0, st, bias, w1,
                     w2, dt_n, u0, target, s + g.us, s + g.qs, loss_ic, s + g.loss_part, n_ics, n_layers,
                     lay);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_resnet_grad_b, dim3(unsigned(g.chunks), unsigned(n_layers)),
                     dim3(kRnLanesB), 0, st, bias, w1, w2, s + g.us, s + g.qs, s + g.part, n_ics,
                     P, lay);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_resnet_grad_c, dim3(grid_for(3 * P + 1, kCBlock)), dim3(kCBlock), 0, st,
                     s + g.part, s + g.loss_part, g.chunks, 3 * P, double(n_ics), grad,
                     loss_mean);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}

}  // extern "C"
