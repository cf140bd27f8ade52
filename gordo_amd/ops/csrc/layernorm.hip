// Grouped LayerNormalization for gfx950: Keras 3 LayerNormalization(axis=-1)
// over the feature axis of a [G, B, Fp] activation, forward and backward.
// Design notes: docs/kernels.md, "Grouped LayerNormalization".
//
//   x, y, dy, dx            [G, B, Fp]  bf16, contiguous
//   gamma, beta, dgamma, dbeta  [G, Fp] fp32
//   mean, rstd              [G, B]      fp32
//
// Fp is the padded width, real_f <= Fp the logical one: every sum runs over
// the real_f logical columns only, whatever the pad columns hold, and pad
// columns get y = dx = dgamma = dbeta = 0 exactly.
//
//   ln_fwd_kernel<L, STORE_STATS, CENTER, SCALE>
//     A row is owned by L lanes (L = 4..64, the power of two >= Fp / 8), one
//     16-byte chunk of 8 bf16 per lane; a wave holds 64 / L rows, a workgroup
//     256 / L. mean and the two-pass variance are L-wide xor butterflies on
//     the register-resident values: no LDS, no barrier.
//   ln_bwd_kernel<L, CENTER, SCALE>
//     grid (G, chunks); a workgroup walks `passes` row groups of its model,
//     the next group's x / dy / mean / rstd in flight while this one is
//     computed. Each lane keeps the fp32 dgamma / dbeta partials of its 8
//     columns in registers over all its rows; the 256 / L row groups of the
//     workgroup meet once, at the end, in an LDS tile of row stride 17 L
//     floats, and the sums go to partial[G, chunks, 2, Fp].
//   ln_param_reduce_kernel
//     sums the chunks in index order into dgamma / dbeta: no atomics, so the
//     result is the same bits on every run.
//
// Loads are never branched around: a dead row or chunk loads a clamped
// (valid) address and is masked where the value is used. `vec` (decided by
// the host: Fp % 8 == 0 and every base 16-byte aligned) selects
// global_load_dwordx4 / global_store_dwordx4; the element arm loads the same
// values one at a time and computes the same bits.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "ln_plan.h"

#define DEV_INLINE __device__ __forceinline__

namespace gordo_ln {

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// sum over the L lanes that own a row (aligned groups of L lanes: a xor
// with m < L stays inside the group; every lane ends with the same bits)
template <int L>
DEV_INLINE float row_sum(float v) {
#pragma unroll
  for (int m = L / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// round to nearest even, NaN kept quiet: the bits __float2bfloat16 gives
DEV_INLINE unsigned bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// 8 bf16 of a row from column c0 (a live chunk's first column, or 0)
DEV_INLINE void load8(const bf16* __restrict__ row, int c0, int Fp, int vec,
                      float (&v)[8]) {
  if (vec) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(row + c0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[2 * q] = __uint_as_float(w[q] << 16);
      v[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u);
    }
  } else {
    const unsigned short* raw = reinterpret_cast<const unsigned short*>(row);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j < Fp ? c0 + j : Fp - 1;
      v[j] = __uint_as_float((unsigned)raw[c] << 16);
    }
  }
}

DEV_INLINE void load8(const float* __restrict__ row, int c0, int Fp, int vec,
                      float (&v)[8]) {
  if (vec) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(row + c0);
    const f32x4 b = *reinterpret_cast<const f32x4*>(row + c0 + 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = a[q], v[4 + q] = b[q];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = row[c0 + j < Fp ? c0 + j : Fp - 1];
  }
}

// the caller has checked that the row and the chunk are live
DEV_INLINE void store8(bf16* __restrict__ row, int c0, int Fp, int vec,
                       const float (&v)[8]) {
  if (vec) {
    u32x4 w;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      w[q] = bf16_bits(v[2 * q]) | (bf16_bits(v[2 * q + 1]) << 16);
    *reinterpret_cast<u32x4*>(row + c0) = w;
  } else {
    unsigned short* raw = reinterpret_cast<unsigned short*>(row);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (c0 + j < Fp) raw[c0 + j] = (unsigned short)bf16_bits(v[j]);
  }
}

// ===========================================================================
// Forward. grid (G, ceil(B / (256 / L))), 256 threads.
// thread t: row group t / L (row blockIdx.y * 256 / L + t / L), chunk t % L
// (columns 8 (t % L) .. + 7).
// ===========================================================================
template <int L, bool STORE_STATS, bool CENTER, bool SCALE>
__global__ __launch_bounds__(THREADS) void ln_fwd_kernel(
    const bf16* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, bf16* __restrict__ y,
    float* __restrict__ mean, float* __restrict__ rstd, int B, int Fp,
    int real_f, float eps, int vec) {
  constexpr int RPB = THREADS / L;
  const int g = blockIdx.x, sub = threadIdx.x % L;
  const int b = blockIdx.y * RPB + threadIdx.x / L;
  const bool live_row = b < B, live_chunk = sub * CHUNK < Fp;
  const int c0 = live_chunk ? sub * CHUNK : 0;
  // columns j < nreal of this lane's chunk are logical
  const int nreal = live_chunk ? real_f - sub * CHUNK : 0;
  const size_t row = ((size_t)g * B + (live_row ? b : B - 1)) * Fp;

  float v[8];
  load8(x + row, c0, Fp, vec, v);
  float ga[8], be[8];
  if (SCALE) load8(gamma + (size_t)g * Fp, c0, Fp, vec, ga);
  if (CENTER) load8(beta + (size_t)g * Fp, c0, Fp, vec, be);

  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = j < nreal ? v[j] : 0.f;
    s += v[j];
  }
  const float mu = row_sum<L>(s) / (float)real_f;
  // two-pass variance on the centred values the output is built from
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = j < nreal ? v[j] - mu : 0.f;
    q += v[j] * v[j];
  }
  const float rs = 1.f / sqrtf(row_sum<L>(q) / (float)real_f + eps);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float o = v[j] * rs;
    if (SCALE) o *= ga[j];
    if (CENTER) o += be[j];
    v[j] = j < nreal ? o : 0.f;
  }
  if (live_row && live_chunk) store8(y + row, c0, Fp, vec, v);
  if (STORE_STATS && live_row && sub == 0) {
    mean[(size_t)g * B + b] = mu;
    rstd[(size_t)g * B + b] = rs;
  }
}

// ===========================================================================
// Backward. grid (G, chunks), 256 threads; workgroup (g, c) owns rows
// [c * passes * RPB, (c + 1) * passes * RPB) of model g.
// LDS tile [RPB][17 L] floats: row group r keeps dgamma of (chunk s, column
// j) at r * 17 L + j * L + s and dbeta 8 L further on. 17 L = L (mod 64), so
// the 64 / L row groups of a wave write L-wide bank ranges side by side for
// every j, and the column sums read consecutive floats: neither side has a
// bank conflict.
// ===========================================================================
template <int L, bool CENTER, bool SCALE>
__global__ __launch_bounds__(THREADS) void ln_bwd_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, bf16* __restrict__ dx,
    float* __restrict__ partial, int B, int Fp, int real_f, int passes,
    int vec) {
  constexpr int RPB = THREADS / L, STRIDE = 17 * L;
  __shared__ float tile[RPB * STRIDE];
  const int g = blockIdx.x, chunk = blockIdx.y, chunks = gridDim.y;
  const int rg = threadIdx.x / L, sub = threadIdx.x % L;
  const bool live_chunk = sub * CHUNK < Fp;
  const int c0 = live_chunk ? sub * CHUNK : 0;
  const int nreal = live_chunk ? real_f - sub * CHUNK : 0;
  const int b0 = chunk * passes * RPB + rg;
  const size_t model = (size_t)g * B;

  float ga[8];
  if (SCALE) load8(gamma + (size_t)g * Fp, c0, Fp, vec, ga);
  float dg[8], db[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dg[j] = db[j] = 0.f;

  // the row in flight: loaded one pass ahead, from a clamped address
  int bn = b0 < B ? b0 : B - 1;
  float xn[8], dn[8];
  load8(x + (model + bn) * Fp, c0, Fp, vec, xn);
  load8(dy + (model + bn) * Fp, c0, Fp, vec, dn);
  float mun = mean[model + bn], rsn = rstd[model + bn];

  for (int p = 0; p < passes; ++p) {
    const int b = b0 + p * RPB;
    const bool live_row = b < B;
    const int nr = live_row ? nreal : 0;
    const size_t row = (model + bn) * Fp;
    float xh[8], dh[8];
    const float mu = mun, rs = rsn;
#pragma unroll
    for (int j = 0; j < 8; ++j) xh[j] = xn[j], dh[j] = dn[j];
    bn = b + RPB < B ? b + RPB : B - 1;
    load8(x + (model + bn) * Fp, c0, Fp, vec, xn);
    load8(dy + (model + bn) * Fp, c0, Fp, vec, dn);
    mun = mean[model + bn], rsn = rstd[model + bn];

    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool m = j < nr;
      const float d = m ? dh[j] : 0.f;
      xh[j] = m ? (xh[j] - mu) * rs : 0.f;
      dh[j] = SCALE ? (m ? d * ga[j] : 0.f) : d;  // pad gamma may be NaN
      s1 += dh[j];
      s2 += dh[j] * xh[j];
      if (SCALE) dg[j] += d * xh[j];
      if (CENTER) db[j] += d;
    }
    const float m1 = row_sum<L>(s1) / (float)real_f;
    const float m2 = row_sum<L>(s2) / (float)real_f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      dh[j] = j < nr ? rs * (dh[j] - m1 - xh[j] * m2) : 0.f;
    if (live_row && live_chunk) store8(dx + row, c0, Fp, vec, dh);
  }

#pragma unroll
  for (int j = 0; j < 8; ++j) {
    tile[rg * STRIDE + j * L + sub] = dg[j];
    tile[rg * STRIDE + 8 * L + j * L + sub] = db[j];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 16 * L; t += THREADS) {
    float s = 0.f;
#pragma unroll 4
    for (int r = 0; r < RPB; ++r) s += tile[r * STRIDE + t];
    const int which = t / (8 * L), rem = t % (8 * L);
    const int col = (rem % L) * CHUNK + rem / L;
    if (col < Fp)
      partial[(((size_t)g * chunks + chunk) * 2 + which) * Fp + col] = s;
  }
}

// partial [G, chunks, 2, Fp] -> dgamma, dbeta [G, Fp] (either may be null),
// chunks summed in index order. grid (G, ceil(2 Fp / 256)).
__global__ __launch_bounds__(THREADS) void ln_param_reduce_kernel(
    const float* __restrict__ partial, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int chunks, int Fp) {
  const int g = blockIdx.x, t = blockIdx.y * THREADS + threadIdx.x;
  if (t >= 2 * Fp) return;
  const int which = t / Fp, col = t % Fp;
  float* out = which == 0 ? dgamma : dbeta;
  if (out == nullptr) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c)
    s += partial[(((size_t)g * chunks + c) * 2 + which) * Fp + col];
  out[(size_t)g * Fp + col] = s;
}

// ---------------------------------------------------------------------------
// Host side: ln_plan.h's plan_layer_norm() decides; the launchers launch the
// plan they get and keep it as the per-thread launch record.
// ---------------------------------------------------------------------------
thread_local LnPlan g_last_ln;

using PlanTuple = std::tuple<std::string, int, bool, int, int, std::string>;

inline PlanTuple plan_tuple(const LnPlan& p, bool launched) {
  return {launched ? p.family_name() : "", p.lanes, p.vec, p.chunks, p.blocks,
          p.error};
}

// (family, lanes, vec, chunks, blocks, error) of a request, without touching
// the GPU; vec is what aligned operands get
PlanTuple layer_norm_plan(bool fwd, int G, int B, int Fp) {
  LnPlan p = plan_layer_norm(fwd, G, B, Fp);
  p.vec = p.ok() && Fp % CHUNK == 0;
  return plan_tuple(p, p.ok());
}

// the same tuple for this thread's last launch; family "" before any
PlanTuple last_layer_norm_launch() {
  return plan_tuple(g_last_ln, g_last_ln.lanes > 0);
}

inline bool aligned16(const torch::Tensor& t) {
  return ((uintptr_t)t.data_ptr() & 15) == 0;
}
inline hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}
// a contiguous bf16 view passes through unchanged, storage offset included
inline torch::Tensor act_operand(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 3, name, " must be [G,B,Fp] on GPU");
  return t.to(torch::kBFloat16).contiguous();
}
// gamma / beta: fp32 [G, Fp], or absent (scale / center off)
inline const float* param_operand(const c10::optional<torch::Tensor>& t,
                                  torch::Tensor& keep, int G, int Fp,
                                  const char* name, bool& vec) {
  if (!t.has_value()) return nullptr;
  keep = t->to(torch::kFloat32).contiguous();
  TORCH_CHECK(keep.is_cuda() && keep.dim() == 2 && keep.size(0) == G &&
                  keep.size(1) == Fp, name, " must be [G,Fp] on GPU");
  vec = vec && aligned16(keep);
  return keep.data_ptr<float>();
}

template <class Fn>
inline void pick_lanes(int lanes, Fn&& f) {
  switch (lanes) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    default: TORCH_CHECK(false, "no LayerNormalization kernel for ", lanes,
                         " lanes per row");
  }
}
template <class Fn>
inline void pick_flag(bool flag, Fn&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

inline LnPlan planned(bool fwd, int G, int B, int Fp, int real_f) {
  LnPlan p = plan_layer_norm(fwd, G, B, Fp);
  TORCH_CHECK(p.ok(), p.error);
  TORCH_CHECK(real_f >= 1 && real_f <= Fp,
              "LayerNormalization needs 1 <= real_f <= Fp, got real_f = ",
              real_f, ", Fp = ", Fp);
  return p;
}

// x [G,B,Fp]; gamma, beta [G,Fp] or None -> {y, mean, rstd} (mean and rstd
// empty without store_stats)
std::vector<torch::Tensor> layer_norm_fwd(torch::Tensor x,
                                          c10::optional<torch::Tensor> gamma,
                                          c10::optional<torch::Tensor> beta,
                                          int64_t real_f, double eps,
                                          bool store_stats) {
  auto xc = act_operand(x, "x");
  const int G = xc.size(0), B = xc.size(1), Fp = xc.size(2);
  LnPlan p = planned(true, G, B, Fp, (int)real_f);
  auto y = torch::empty({G, B, Fp}, xc.options());
  bool vec = Fp % CHUNK == 0 && aligned16(xc) && aligned16(y);
  torch::Tensor gk, bk;
  const float* gp = param_operand(gamma, gk, G, Fp, "gamma", vec);
  const float* bp = param_operand(beta, bk, G, Fp, "beta", vec);
  auto fopts = xc.options().dtype(torch::kFloat32);
  auto mean = torch::empty({store_stats ? G : 0, store_stats ? B : 0}, fopts);
  auto rstd = torch::empty_like(mean);
  p.vec = vec;
  g_last_ln = p;
  pick_lanes(p.lanes, [&](auto L) {
    pick_flag(store_stats, [&](auto ST) {
      pick_flag(bp != nullptr, [&](auto CE) {
        pick_flag(gp != nullptr, [&](auto SC) {
          hipLaunchKernelGGL(
              (ln_fwd_kernel<decltype(L)::value, decltype(ST)::value,
                             decltype(CE)::value, decltype(SC)::value>),
              dim3(G, p.chunks), dim3(THREADS), 0, cur_stream(),
              (const bf16*)xc.data_ptr(), gp, bp, (bf16*)y.data_ptr(),
              store_stats ? mean.data_ptr<float>() : nullptr,
              store_stats ? rstd.data_ptr<float>() : nullptr, B, Fp,
              (int)real_f, (float)eps, vec ? 1 : 0);
        });
      });
    });
  });
  return {y, mean, rstd};
}

// dy, x [G,B,Fp]; mean, rstd [G,B]; gamma [G,Fp] or None -> {dx, dgamma,
// dbeta} (dgamma empty without gamma, dbeta empty without center)
std::vector<torch::Tensor> layer_norm_bwd(torch::Tensor dy, torch::Tensor x,
                                          torch::Tensor mean,
                                          torch::Tensor rstd,
                                          c10::optional<torch::Tensor> gamma,
                                          int64_t real_f, bool center) {
  auto dc = act_operand(dy, "dy"), xc = act_operand(x, "x");
  const int G = xc.size(0), B = xc.size(1), Fp = xc.size(2);
  TORCH_CHECK(dc.sizes() == xc.sizes(), "dy does not match x");
  auto mc = mean.to(torch::kFloat32).contiguous();
  auto rc = rstd.to(torch::kFloat32).contiguous();
  TORCH_CHECK(mc.is_cuda() && rc.is_cuda() && mc.dim() == 2 &&
                  mc.size(0) == G && mc.size(1) == B &&
                  rc.sizes() == mc.sizes(), "mean, rstd must be [G,B] on GPU");
  LnPlan p = planned(false, G, B, Fp, (int)real_f);
  auto dx = torch::empty({G, B, Fp}, xc.options());
  bool vec =
      Fp % CHUNK == 0 && aligned16(xc) && aligned16(dc) && aligned16(dx);
  torch::Tensor gk;
  const float* gp = param_operand(gamma, gk, G, Fp, "gamma", vec);
  auto fopts = xc.options().dtype(torch::kFloat32);
  auto partial = torch::empty({G, p.chunks, 2, Fp}, fopts);
  auto dgamma = torch::empty({gp ? G : 0, gp ? Fp : 0}, fopts);
  auto dbeta = torch::empty({center ? G : 0, center ? Fp : 0}, fopts);
  p.vec = vec;
  g_last_ln = p;
  pick_lanes(p.lanes, [&](auto L) {
    pick_flag(center, [&](auto CE) {
      pick_flag(gp != nullptr, [&](auto SC) {
        hipLaunchKernelGGL(
            (ln_bwd_kernel<decltype(L)::value, decltype(CE)::value,
                           decltype(SC)::value>),
            dim3(G, p.chunks), dim3(THREADS), 0, cur_stream(),
            (const bf16*)dc.data_ptr(), (const bf16*)xc.data_ptr(),
            mc.data_ptr<float>(), rc.data_ptr<float>(), gp,
            (bf16*)dx.data_ptr(), partial.data_ptr<float>(), B, Fp,
            (int)real_f, p.passes, vec ? 1 : 0);
      });
    });
  });
  if (gp != nullptr || center)
    hipLaunchKernelGGL(ln_param_reduce_kernel,
                       dim3(G, ceil_div(2 * Fp, THREADS)), dim3(THREADS), 0,
                       cur_stream(), partial.data_ptr<float>(),
                       gp ? dgamma.data_ptr<float>() : nullptr,
                       center ? dbeta.data_ptr<float>() : nullptr, p.chunks,
                       Fp);
  return {dx, dgamma, dbeta};
}

}  // namespace gordo_ln
