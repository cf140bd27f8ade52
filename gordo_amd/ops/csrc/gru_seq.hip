// Fused GRU sequence-scan kernels for MI355X (gfx950): the Keras 3 GRU
// cell with reset_after=True, gate order z, r, n along the 3H axis and a
// two-row bias (row 0 joins x @ Wx, row 1 joins h @ Wh):
//
//   z = σ(mx_z + mh_z)      r = σ(mx_r + mh_r)
//   n = tanh(mx_n + r ⊙ mh_n)
//   h_t = z ⊙ h_{t-1} + (1 − z) ⊙ n
//
// The recurrent half of the candidate gate (q = mh_n) has to stay apart
// from the x half until r is known, so the LSTM scans' "one [h | x] MFMA
// loop, then a pointwise phase" does not carry over as it stands. Both
// kernels here keep that loop shape by contracting over a FOUR-block
// column space {z, r, n_x, n_h} whose last two blocks are zero in the
// half of K they do not use; k-steps that are zero for a whole 16-column
// tile are skipped on block-uniform values.
//
//   gru_seq_fwd_kernel : per (model g, row tile) workgroup the whole
//     T loop on device; writes hs and, for training, gacts = {z, r, n, q}.
//   gru_seq_bwd_kernel : the reverse-time scan; writes the kernel-side
//     gate grads dGx = [da_z, da_r, da_n], the recurrent-side ones
//     dGh = [da_z, da_r, dq] and optionally dX = dGx @ Wx^T.
//
// Geometry: 8 <= H <= 64, H % 8 == 0, 8 <= F <= 128, F % 8 == 0,
// T < 2^17. One workgroup = 4 waves. docs/kernels.md, "Fused GRU scan".
//
// Wider layers (the fused forward keeps 4H weight rows in LDS: 200 KB at
// (H, F) = (128, 56)) run on a second, two-step pair further down:
//
//   gru_seq_fwd_big_kernel : the scan on mx = x @ Wx + b[0], a grouped
//     GEMM made by the entry; Wh streamed from L2, gate phase in registers.
//   gru_seq_bwd_big_kernel : the reverse scan to dGx / dGh; dX is a
//     grouped GEMM made by the entry.
//
// Geometry: 16 <= H <= 256, H % 16 == 0, any F % 8 == 0, T < 2^17.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "scan_plan.h"

#define DEV_INLINE __device__ __forceinline__

// the grouped GEMMs around the two-step scans (gordo_kernels.hip)
namespace gordo_gemm {
torch::Tensor linear_fwd(torch::Tensor X, torch::Tensor W, torch::Tensor b);
torch::Tensor linear_bwd_data(torch::Tensor dZ, torch::Tensor W);
}  // namespace gordo_gemm

namespace gordo_gru {

// Device code of this file is built without packed fp32 instructions
// (v_pk_{add,mul,fma}_f32): the two-units-per-thread gate phase below is
// exactly the shape the compiler would pack.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

DEV_INLINE float bf2f(bf16 v) { return __bfloat162float(v); }
DEV_INLINE bf16 f2bf(float v) { return __float2bfloat16(v); }
DEV_INLINE unsigned pack2(float a, float b) {
  return (unsigned)__builtin_bit_cast(unsigned short, f2bf(a)) |
         ((unsigned)__builtin_bit_cast(unsigned short, f2bf(b)) << 16);
}
DEV_INLINE float lo_f(unsigned p) { return __uint_as_float(p << 16); }
DEV_INLINE float hi_f(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
DEV_INLINE float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }
DEV_INLINE float fast_tanhf_(float x) {
  float e = __expf(2.f * x);
  return 1.f - 2.f / (e + 1.f);  // saturates to 1 when e overflows to inf
}

constexpr int GATE_PAD = gordo_lstm::GRU_GATE_PAD;

// ===========================================================================
// Forward scan.
//   xseq  [G, B, T, F]   bf16
//   WcatT [G, 4H, Kc]    bf16, Kc = H + F, K order [h | x]; column groups
//                        z, r (whole K), n_x (h rows zero), n_h (x rows zero)
//   bias4 [G, 4H]        f32: b0+b1 for z and r, b0_n for n_x, b1_n for n_h
//   hs    [G, B, T, H]   bf16 out
//   gacts [G, B, T, 4H]  bf16 out {z, r, n, q} (STORE_AUX)
// LDS: WT [4H][LDKc] bf16 | hxS [ROWS][LDKc] bf16 | gS [ROWS][4H+4] f32 |
//      bS [4H] f32. The single h state is the bf16 h section of hxS: the
// value that enters the next step's MFMA, the convex mix and hs is one and
// the same, which is also what the backward scan reads back as h_{t-1}.
// The gate tile gS stays fp32 (h_t is a convex mix of h_{t-1} and n: a
// rounding of mh_n would enter every later step undamped).
// ===========================================================================
template <int ROWS, bool STORE_AUX>
__global__ __launch_bounds__(256) void gru_seq_fwd_kernel(
    const bf16* __restrict__ xseq, const bf16* __restrict__ WcatT,
    const float* __restrict__ bias4, bf16* __restrict__ hs,
    bf16* __restrict__ gacts, int B, int T, int H, int F) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H4 = 4 * H;
  const int Kc = H + F;  // both % 8 == 0
  // K row padded to the MFMA K step (zeros staged beyond Kc)
  const int LDKc = ((Kc + 31) & ~31) + 8;
  // 4H + 4 floats: rows 4 apart (the MFMA epilogue's kslot stride) land
  // 16 banks apart
  const int LDGF = H4 + GATE_PAD;
  bf16* WT = reinterpret_cast<bf16*>(smem);                    // [H4][LDKc]
  bf16* hxS = WT + (size_t)H4 * LDKc;                          // [ROWS][LDKc]
  float* gS = reinterpret_cast<float*>(hxS + (size_t)ROWS * LDKc);
  float* bS = gS + (size_t)ROWS * LDGF;                        // [H4]

  const int nb = (B + ROWS - 1) / ROWS;
  const int g = blockIdx.x / nb;
  const int r0 = (blockIdx.x % nb) * ROWS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15;
  const int kslot = lane >> 4;

  const bf16* WTg = WcatT + (size_t)g * H4 * Kc;
  const bf16* xg = xseq + ((size_t)g * B + r0) * T * F;
  bf16* hsg = hs + ((size_t)g * B + r0) * T * H;
  bf16* gag = gacts + ((size_t)g * B + r0) * T * H4;
  const int rows_here = min(ROWS, B - r0);

  // ---- stage weights (16-byte chunks, zero K tail) and bias ----
  const int CW = LDKc / 8, CK = Kc / 8;
  for (int i = tid; i < H4 * CW; i += 256) {
    int n = i / CW, c = i % CW;
    bf16x8 v = {};
    if (c < CK)
      v = *reinterpret_cast<const bf16x8*>(&WTg[(size_t)n * Kc + c * 8]);
    *reinterpret_cast<bf16x8*>(&WT[(size_t)n * LDKc + c * 8]) = v;
  }
  for (int i = tid; i < H4; i += 256) bS[i] = bias4[(size_t)g * H4 + i];
  // zero the h section and the K tail ONLY: the x section is written by
  // other threads in the x_0 loop below, zeroing it here would race
  for (int i = tid; i < ROWS * CW; i += 256) {
    int row = i / CW, c = i % CW;
    if (c < H / 8 || c >= CK) {
      bf16x8 zero = {};
      *reinterpret_cast<bf16x8*>(&hxS[row * LDKc + c * 8]) = zero;
    }
  }
  const int F8 = F / 8;
  for (int i = tid; i < ROWS * F8; i += 256) {
    int row = i / F8, f8 = i % F8;
    bf16x8 v = {};
    if (row < rows_here)
      v = *reinterpret_cast<const bf16x8*>(&xg[(size_t)row * T * F + f8 * 8]);
    *reinterpret_cast<bf16x8*>(&hxS[row * LDKc + H + f8 * 8]) = v;
  }
  __syncthreads();

  constexpr int FM = ROWS / 16;
  const int wcol0 = wid * 64;
  // k range of each 16-column tile of this wave (block-uniform): a tile
  // inside n_x has zero weights on the h rows, one inside n_h on the x
  // rows, one beyond 4H has no columns at all
  int klo[4], khi[4];
  #pragma unroll
  for (int fn = 0; fn < 4; ++fn) {
    const int c0 = wcol0 + fn * 16, c1 = c0 + 16;
    klo[fn] = (c0 >= 2 * H && c1 <= 3 * H) ? (H & ~31) : 0;
    khi[fn] = c0 >= H4 ? 0 : (c0 >= 3 * H ? ((H + 31) & ~31) : Kc);
  }
  // per-thread x-prefetch slots (strided like the staging loop)
  constexpr int NPF = (ROWS * 16 + 255) / 256;  // F/8 <= 16
  bf16x8 xpf[NPF];
  const int nx = ROWS * F8;
  const int H2 = H / 2;

  for (int t = 0; t < T; ++t) {
    // ---- pre-activations = [h | x_t] @ WT^T + bias4 (MFMA over Kc) ----
    if (khi[0] > 0) {
      f32x4 acc[FM][4] = {};
      for (int kk = 0; kk < Kc; kk += 32) {
        bf16x8 a[FM];
        #pragma unroll
        for (int fm = 0; fm < FM; ++fm)
          a[fm] = *reinterpret_cast<const bf16x8*>(
              &hxS[(fm * 16 + l15) * LDKc + kk + kslot * 8]);
        #pragma unroll
        for (int fn = 0; fn < 4; ++fn) {
          if (kk < klo[fn] || kk >= khi[fn]) continue;  // block-uniform
          int col = min(wcol0 + fn * 16 + l15, H4 - 1);
          bf16x8 b = *reinterpret_cast<const bf16x8*>(
              &WT[(size_t)col * LDKc + kk + kslot * 8]);
          #pragma unroll
          for (int fm = 0; fm < FM; ++fm)
            acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[fm], b, acc[fm][fn], 0, 0, 0);
        }
      }
      #pragma unroll
      for (int fn = 0; fn < 4; ++fn) {
        int col = wcol0 + fn * 16 + l15;
        if (col >= H4) continue;
        float bv = bS[col];
        #pragma unroll
        for (int fm = 0; fm < FM; ++fm) {
          #pragma unroll
          for (int r = 0; r < 4; ++r) {
            int row = fm * 16 + kslot * 4 + r;
            gS[row * LDGF + col] = acc[fm][fn][r] + bv;
          }
        }
      }
    }
    __syncthreads();

    // ---- register-prefetch x_{t+1} (no dependence on this step) ----
    if (t + 1 < T) {
      #pragma unroll
      for (int s = 0; s < NPF; ++s) {
        int i = tid + s * 256;
        if (i < nx) {
          int row = i / F8, f8 = i % F8;
          bf16x8 v = {};
          if (row < rows_here)
            v = *reinterpret_cast<const bf16x8*>(
                &xg[((size_t)row * T + (t + 1)) * F + f8 * 8]);
          xpf[s] = v;
        }
      }
    }

    // ---- gate math, two hidden units per thread ----
    for (int e = tid; e < ROWS * H2; e += 256) {
      int row = e / H2, hh = (e % H2) * 2;
      const float* gr = &gS[row * LDGF + hh];
      float2 az = *reinterpret_cast<const float2*>(gr);
      float2 ar = *reinterpret_cast<const float2*>(gr + H);
      float2 an = *reinterpret_cast<const float2*>(gr + 2 * H);
      float2 q = *reinterpret_cast<const float2*>(gr + 3 * H);
      unsigned* hp = reinterpret_cast<unsigned*>(&hxS[row * LDKc + hh]);
      const unsigned hprev = *hp;
      float z0 = sigmoidf_(az.x), z1 = sigmoidf_(az.y);
      float r0_ = sigmoidf_(ar.x), r1_ = sigmoidf_(ar.y);
      float n0 = fast_tanhf_(an.x + r0_ * q.x);
      float n1 = fast_tanhf_(an.y + r1_ * q.y);
      float h0 = z0 * lo_f(hprev) + (1.f - z0) * n0;
      float h1 = z1 * hi_f(hprev) + (1.f - z1) * n1;
      const unsigned hnew = pack2(h0, h1);
      *hp = hnew;
      if (row < rows_here) {
        size_t rt = (size_t)row * T + t;
        *reinterpret_cast<unsigned*>(&hsg[rt * H + hh]) = hnew;
        if (STORE_AUX) {
          bf16* ga = &gag[rt * H4 + hh];
          *reinterpret_cast<unsigned*>(ga) = pack2(z0, z1);
          *reinterpret_cast<unsigned*>(ga + H) = pack2(r0_, r1_);
          *reinterpret_cast<unsigned*>(ga + 2 * H) = pack2(n0, n1);
          *reinterpret_cast<unsigned*>(ga + 3 * H) = pack2(q.x, q.y);
        }
      }
    }
    // x_{t+1} into the K-buffer's x section before the barrier (the gate
    // phase does not read that section)
    if (t + 1 < T) {
      #pragma unroll
      for (int s = 0; s < NPF; ++s) {
        int i = tid + s * 256;
        if (i < nx) {
          int row = i / F8, f8 = i % F8;
          *reinterpret_cast<bf16x8*>(&hxS[row * LDKc + H + f8 * 8]) = xpf[s];
        }
      }
    }
    __syncthreads();
  }
}

// ===========================================================================
// Backward (reverse-time) scan.
//   dSeq  [G, B, T, H] bf16 (or [G, B, H] with LAST_ONLY)
//   gacts [G, B, T, 4H] bf16 {z, r, n, q};  hs [G, B, T, H] bf16
//   Wh [G, H, 3H], Wx [G, F, 3H] bf16 (native layout; Wx with HAS_DX)
//   dGx, dGh [G, B, T, 3H] bf16 out;  dX [G, B, T, F] bf16 out (HAS_DX)
// LDS: WN [H+Fx][ldg] bf16 | dgS [ROWS][ldg] bf16 | cS [ROWS][H] f32 |
//      tile [ROWS][CPR*16 bytes] | xS [ROWS][F] bf16.
// dgS holds FOUR blocks {da_z, da_r, da_n, dq}. A Wh row is staged as
// [Wh_z, Wh_r, 0, Wh_n] and a Wx row as [Wx_z, Wx_r, Wx_n, 0], so one
// MFMA phase over K = 4H gives carry = dGh @ Wh^T in the first H output
// columns and dX = dGx @ Wx^T in the next F; the k-steps inside a tile's
// zero block are skipped. cS is the fp32 carry: the gate phase leaves
// dh ⊙ z in it and the MFMA epilogue adds dGh @ Wh^T.
// The step tile {gacts_t, hs_{t-1}, dSeq_t} of step t-1 is fetched into
// registers right after step t's gate phase (16-byte chunks, clamped
// addresses, no branch around a load), left untouched during the MFMA
// phase and the dG stores, and written to the single LDS tile before the
// step's second barrier: one step of look-ahead, no ring.
// ===========================================================================
template <int ROWS, bool HAS_DX, bool LAST_ONLY>
__global__ __launch_bounds__(256) void gru_seq_bwd_kernel(
    const bf16* __restrict__ dSeq, const bf16* __restrict__ gacts,
    const bf16* __restrict__ hs, const bf16* __restrict__ Wh,
    const bf16* __restrict__ Wx, bf16* __restrict__ dGx,
    bf16* __restrict__ dGh, bf16* __restrict__ dX, int B, int T, int H,
    int F, int ldg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H3 = 3 * H, H4 = 4 * H;
  const int Fx = HAS_DX ? F : 0;
  const int HF = H + Fx;
  const int H8 = H / 8;
  // 16-byte chunks per tile row: 4H gacts, H h_prev, H dSeq (all bf16)
  const int CPR = H8 * (LAST_ONLY ? 5 : 6);
  const int RS = CPR * 16;
  bf16* WN = reinterpret_cast<bf16*>(smem);                 // [HF][ldg]
  bf16* dgS = WN + (size_t)HF * ldg;                        // [ROWS][ldg]
  float* cS = reinterpret_cast<float*>(dgS + (size_t)ROWS * ldg);
  char* tile = reinterpret_cast<char*>(cS + (size_t)ROWS * H);
  bf16* xS = reinterpret_cast<bf16*>(tile + (size_t)ROWS * RS);

  const int nb = (B + ROWS - 1) / ROWS;
  const int g = blockIdx.x / nb;
  const int r0 = (blockIdx.x % nb) * ROWS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15;
  const int kslot = lane >> 4;

  const bf16* gag = gacts + ((size_t)g * B + r0) * T * H4;
  const bf16* hsg = hs + ((size_t)g * B + r0) * T * H;
  const bf16* dSg = LAST_ONLY ? dSeq + ((size_t)g * B + r0) * H
                              : dSeq + ((size_t)g * B + r0) * T * H;
  bf16* dGxg = dGx + ((size_t)g * B + r0) * T * H3;
  bf16* dGhg = dGh + ((size_t)g * B + r0) * T * H3;
  bf16* dXg = HAS_DX ? dX + ((size_t)g * B + r0) * T * F : nullptr;
  const int rows_here = min(ROWS, B - r0);

  // ---- per-thread tile slots: address = lsrc + max(t, lmin) * lstr.
  // The h_prev slots point one step before the row (lmin = 1 keeps them
  // inside it: step 0 reads hs_0 and the gate phase takes zero instead)
  constexpr int MAXS = (ROWS * (LAST_ONLY ? 40 : 48) + 255) / 256;
  const int total = ROWS * CPR;
  const char* lsrc[MAXS];
  int lstr[MAXS], lmin[MAXS];
  u32x4 R[MAXS];
  #pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    int c = min(tid + s * 256, total - 1);
    int row = min(c / CPR, rows_here - 1), j = c % CPR;
    size_t rt = (size_t)row * T;
    if (j < 4 * H8) {
      lsrc[s] = reinterpret_cast<const char*>(gag + rt * H4 + j * 8);
      lstr[s] = H4 * 2;
      lmin[s] = 0;
    } else if (j < 5 * H8) {
      lsrc[s] = reinterpret_cast<const char*>(hsg + rt * H + (j - 4 * H8) * 8) -
                (ptrdiff_t)H * 2;
      lstr[s] = H * 2;
      lmin[s] = 1;
    } else {
      lsrc[s] = reinterpret_cast<const char*>(dSg + rt * H + (j - 5 * H8) * 8);
      lstr[s] = H * 2;
      lmin[s] = 0;
    }
  }
  auto load_tile = [&](int tt) {
    #pragma unroll
    for (int s = 0; s < MAXS; ++s)
      R[s] = *reinterpret_cast<const u32x4*>(
          lsrc[s] + (size_t)max(tt, lmin[s]) * lstr[s]);
  };
  auto write_tile = [&]() {
    #pragma unroll
    for (int s = 0; s < MAXS; ++s) {
      int c = tid + s * 256;
      if (c < total) *reinterpret_cast<u32x4*>(tile + c * 16) = R[s];
    }
  };

  // ---- per-thread dGx / dGh / dX store slots (element offsets at t = 0);
  // row < rows_here <= ROWS bounds the chunk index too
  constexpr int DGS = (ROWS * 24 + 255) / 256;  // ROWS * (3H/8) at H = 64
  int dgx_src[DGS], dgh_src[DGS], dg_dst[DGS];
  #pragma unroll
  for (int s = 0; s < DGS; ++s) {
    int qd = tid + s * 256;
    int row = qd / (3 * H8), j = qd % (3 * H8);
    bool ok = row < rows_here;
    dgx_src[s] = ok ? row * ldg + j * 8 : -1;
    dgh_src[s] = row * ldg + (j < 2 * H8 ? j : j + H8) * 8;
    dg_dst[s] = ok ? row * T * H3 + j * 8 : 0;
  }
  constexpr int DXS = HAS_DX ? ROWS / 16 : 1;  // ROWS * (F/8) at F = 128
  int dx_dst[DXS];
  #pragma unroll
  for (int s = 0; s < DXS; ++s) {
    int qd = tid + s * 256;
    int f8 = HAS_DX ? F / 8 : 1;
    int row = qd / f8, j = qd % f8;
    dx_dst[s] = (HAS_DX && row < rows_here) ? row * T * F + j * 8 : -1;
  }

  // ---- stage weights, zero dgS, seed the carry, land tile T-1 ----
  load_tile(T - 1);
  const int CG = ldg / 8;
  {
    const bf16* Whg = Wh + (size_t)g * H * H3;
    for (int i = tid; i < H * CG; i += 256) {
      int h = i / CG, c = i % CG;
      bf16x8 v = {};
      if (c < 2 * H8)
        v = *reinterpret_cast<const bf16x8*>(&Whg[(size_t)h * H3 + c * 8]);
      else if (c >= 3 * H8 && c < 4 * H8)
        v = *reinterpret_cast<const bf16x8*>(
            &Whg[(size_t)h * H3 + (c - H8) * 8]);
      *reinterpret_cast<bf16x8*>(&WN[(size_t)h * ldg + c * 8]) = v;
    }
  }
  if (HAS_DX) {
    const bf16* Wxg = Wx + (size_t)g * F * H3;
    bf16* WxN = WN + (size_t)H * ldg;
    for (int i = tid; i < F * CG; i += 256) {
      int f = i / CG, c = i % CG;
      bf16x8 v = {};
      if (c < 3 * H8)
        v = *reinterpret_cast<const bf16x8*>(&Wxg[(size_t)f * H3 + c * 8]);
      *reinterpret_cast<bf16x8*>(&WxN[(size_t)f * ldg + c * 8]) = v;
    }
  }
  for (int i = tid; i < ROWS * CG; i += 256) {
    bf16x8 zero = {};
    *reinterpret_cast<bf16x8*>(&dgS[i * 8]) = zero;
  }
  for (int i = tid; i < ROWS * H; i += 256) {
    int row = i / H, col = i % H;
    float v = 0.f;
    if (LAST_ONLY && row < rows_here) v = bf2f(dSg[(size_t)row * H + col]);
    cS[i] = v;
  }
  write_tile();
  __syncthreads();

  constexpr int FM = ROWS / 16;
  const int n_items = FM * ((HF + 15) / 16);

  for (int t = T - 1; t >= 0; --t) {
    // ---- pointwise gate backward, operands from the tile ----
    for (int e = tid; e < ROWS * H; e += 256) {
      int row = e / H, hh = e % H;
      const bf16* gp = reinterpret_cast<const bf16*>(tile + row * RS);
      float z = bf2f(gp[hh]);
      float r = bf2f(gp[H + hh]);
      float n = bf2f(gp[2 * H + hh]);
      float q = bf2f(gp[3 * H + hh]);
      float hp = bf2f(gp[H4 + hh]);
      hp = (t > 0) ? hp : 0.f;
      float dh = cS[row * H + hh];
      if (!LAST_ONLY) dh += bf2f(gp[H4 + H + hh]);
      float dan = dh * (1.f - z) * (1.f - n * n);
      float daz = dh * (hp - n) * z * (1.f - z);
      float dar = dan * q * r * (1.f - r);
      float dq = dan * r;
      cS[row * H + hh] = dh * z;
      bf16* dg = &dgS[row * ldg + hh];
      dg[0] = f2bf(daz);
      dg[H] = f2bf(dar);
      dg[2 * H] = f2bf(dan);
      dg[3 * H] = f2bf(dq);
    }
    __syncthreads();

    // ---- issue the fetch of step t-1; used only at write_tile below ----
    load_tile(t - 1);

    // ---- [carry | dX_t] = dgS @ WN^T, one 16x16 output tile per item ----
    for (int item = wid; item < n_items; item += 4) {
      const int fm = item % FM, c0 = (item / FM) * 16;
      const bool all_h = c0 + 16 <= H, all_x = c0 >= H;  // block-uniform
      const int col = min(c0 + l15, HF - 1);
      f32x4 acc = {};
      for (int kk = 0; kk < H4; kk += 32) {
        if (all_h && kk >= 2 * H && kk + 32 <= H3) continue;  // zero block
        if (all_x && kk >= H3) continue;                      // zero block
        bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &dgS[(fm * 16 + l15) * ldg + kk + kslot * 8]);
        bf16x8 b = *reinterpret_cast<const bf16x8*>(
            &WN[(size_t)col * ldg + kk + kslot * 8]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
      }
      const int oc = c0 + l15;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = fm * 16 + kslot * 4 + r;
        if (oc < H) {
          cS[row * H + oc] += acc[r];
        } else if (HAS_DX && oc < HF) {
          xS[row * F + (oc - H)] = f2bf(acc[r]);
        }
      }
    }

    // ---- this step's dGx / dGh from dgS, then land tile t-1 ----
    #pragma unroll
    for (int s = 0; s < DGS; ++s) {
      if (dgx_src[s] >= 0) {
        size_t dst = (size_t)dg_dst[s] + (size_t)t * H3;
        *reinterpret_cast<u32x4*>(dGxg + dst) =
            *reinterpret_cast<const u32x4*>(dgS + dgx_src[s]);
        *reinterpret_cast<u32x4*>(dGhg + dst) =
            *reinterpret_cast<const u32x4*>(dgS + dgh_src[s]);
      }
    }
    write_tile();
    __syncthreads();

    // ---- dX of this step from the staging tile (the next MFMA epilogue
    // rewrites it only after the next barrier) ----
    if (HAS_DX) {
      #pragma unroll
      for (int s = 0; s < DXS; ++s) {
        if (dx_dst[s] >= 0) {
          *reinterpret_cast<u32x4*>(dXg + (size_t)dx_dst[s] + (size_t)t * F) =
              *reinterpret_cast<const u32x4*>(xS + (tid + s * 256) * 8);
        }
      }
    }
  }
}

// ===========================================================================
// Two-step scans (H % 16 == 0, 16 <= H <= 256; the x side is a grouped
// GEMM outside). Wh stays in global memory (L2-resident after the first
// step) and is the MFMA *A* operand: 16 hidden units per fragment,
// K-contiguous 16-byte loads. The B operand is 16 batch rows of the
// recurrent state from LDS. The 16x16x32 accumulator then gives a lane
// four CONSECUTIVE hidden units (kslot * 4 ..) of ONE batch row (l15), so
// the whole gate phase runs on the accumulators with 8-byte accesses: no
// gate tile, no staging tile. A work item is one 16-unit tile u with the
// accumulators of all ROWS/16 row blocks: the weight fragments of a k-step
// are loaded once and used ROWS/16 times. Tiles are dealt round-robin to
// the four waves (wave index through readfirstlane: every branch around
// an MFMA is wave-uniform). The state is ping-ponged: a step reads buffer
// `step & 1` and writes the other, so one barrier per step is enough.
// Rows past rows_here load from the last live row's addresses, compute,
// and store nothing.
//
// Forward.
//   mx   [G, B, T, 3H] bf16 = x @ Wx + b[0]
//   WhT  [G, 3H, Kp]   bf16, Kp = round32(H), zero K tail
//   bh   [G, 3H]       f32 = b[1]
//   hs   [G, B, T, H], gacts [G, B, T, 4H] bf16 out (gacts: STORE_AUX)
// LDS: hS [2][ROWS][Kp + 8] bf16; columns [H, Kp + 8) are zeroed once and
// never written.
// ===========================================================================
DEV_INLINE void unpack4(uint2 p, float (&v)[4]) {
  v[0] = lo_f(p.x); v[1] = hi_f(p.x); v[2] = lo_f(p.y); v[3] = hi_f(p.y);
}
DEV_INLINE uint2 pack4(const float (&v)[4]) {
  return make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
}
DEV_INLINE uint2 ld8(const bf16* p) {
  return *reinterpret_cast<const uint2*>(p);
}
DEV_INLINE void st8(bf16* p, uint2 v) { *reinterpret_cast<uint2*>(p) = v; }

template <int ROWS, bool STORE_AUX>
__global__ __launch_bounds__(256) void gru_seq_fwd_big_kernel(
    const bf16* __restrict__ mx, const bf16* __restrict__ WhT,
    const float* __restrict__ bh, bf16* __restrict__ hs,
    bf16* __restrict__ gacts, int B, int T, int H, int Kp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H3 = 3 * H, H4 = 4 * H;
  const int LDH = Kp + 8;
  bf16* hS = reinterpret_cast<bf16*>(smem);  // [2][ROWS][LDH]

  const int nb = (B + ROWS - 1) / ROWS;
  const int g = blockIdx.x / nb;
  const int r0 = (blockIdx.x % nb) * ROWS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15;
  const int kslot = lane >> 4;

  const bf16* WTg = WhT + (size_t)g * H3 * Kp;
  const float* bg = bh + (size_t)g * H3;
  const bf16* mxg = mx + ((size_t)g * B + r0) * T * H3;
  bf16* hsg = hs + ((size_t)g * B + r0) * T * H;
  bf16* gag = gacts + ((size_t)g * B + r0) * T * H4;
  const int rows_here = min(ROWS, B - r0);

  for (int i = tid; i < 2 * ROWS * LDH / 8; i += 256) {
    bf16x8 zero = {};
    *reinterpret_cast<bf16x8*>(&hS[i * 8]) = zero;
  }
  __syncthreads();

  constexpr int FM = ROWS / 16;
  const int NT = H / 16;
  // this lane's batch row of each row block, clamped for the loads
  size_t rowT[FM];
  #pragma unroll
  for (int fm = 0; fm < FM; ++fm)
    rowT[fm] = (size_t)min(fm * 16 + l15, rows_here - 1) * T;

  for (int t = 0; t < T; ++t) {
    const bf16* hc = hS + (size_t)(t & 1) * ROWS * LDH;
    bf16* hn = hS + (size_t)((t & 1) ^ 1) * ROWS * LDH;
    for (int u = wid; u < NT; u += 4) {
      const int unit = u * 16 + kslot * 4;
      // x-side pre-activations of this step: issued above the K loop,
      // untouched until the epilogue
      uint2 xz[FM], xr[FM], xn[FM];
      #pragma unroll
      for (int fm = 0; fm < FM; ++fm) {
        const bf16* p = mxg + (rowT[fm] + t) * H3 + unit;
        xz[fm] = ld8(p);
        xr[fm] = ld8(p + H);
        xn[fm] = ld8(p + 2 * H);
      }
      const float4 bz4 = *reinterpret_cast<const float4*>(bg + unit);
      const float4 br4 = *reinterpret_cast<const float4*>(bg + H + unit);
      const float4 bq4 = *reinterpret_cast<const float4*>(bg + 2 * H + unit);

      f32x4 az[FM] = {}, ar[FM] = {}, aq[FM] = {};
      const bf16* wz = WTg + (size_t)(u * 16 + l15) * Kp + kslot * 8;
      const bf16* wr_ = wz + (size_t)H * Kp;
      const bf16* wq = wr_ + (size_t)H * Kp;
      const bf16* hb = hc + l15 * LDH + kslot * 8;
      for (int kk = 0; kk < Kp; kk += 32) {
        bf16x8 fz = *reinterpret_cast<const bf16x8*>(wz + kk);
        bf16x8 fr = *reinterpret_cast<const bf16x8*>(wr_ + kk);
        bf16x8 fq = *reinterpret_cast<const bf16x8*>(wq + kk);
        #pragma unroll
        for (int fm = 0; fm < FM; ++fm) {
          bf16x8 b = *reinterpret_cast<const bf16x8*>(hb + fm * 16 * LDH + kk);
          az[fm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fz, b, az[fm], 0, 0, 0);
          ar[fm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr, b, ar[fm], 0, 0, 0);
          aq[fm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq, b, aq[fm], 0, 0, 0);
        }
      }

      const float bz[4] = {bz4.x, bz4.y, bz4.z, bz4.w};
      const float br[4] = {br4.x, br4.y, br4.z, br4.w};
      const float bq[4] = {bq4.x, bq4.y, bq4.z, bq4.w};
      #pragma unroll
      for (int fm = 0; fm < FM; ++fm) {
        const int row = fm * 16 + l15;
        float mz[4], mr[4], mn[4], hp[4], z[4], r[4], n[4], q[4], h[4];
        unpack4(xz[fm], mz);
        unpack4(xr[fm], mr);
        unpack4(xn[fm], mn);
        unpack4(ld8(hc + row * LDH + unit), hp);
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
          z[j] = sigmoidf_(mz[j] + az[fm][j] + bz[j]);
          r[j] = sigmoidf_(mr[j] + ar[fm][j] + br[j]);
          q[j] = aq[fm][j] + bq[j];
          n[j] = fast_tanhf_(mn[j] + r[j] * q[j]);
          h[j] = z[j] * hp[j] + (1.f - z[j]) * n[j];
        }
        const uint2 hnew = pack4(h);
        st8(hn + row * LDH + unit, hnew);
        if (row < rows_here) {
          const size_t rt = (size_t)row * T + t;
          st8(hsg + rt * H + unit, hnew);
          if (STORE_AUX) {
            bf16* ga = gag + rt * H4 + unit;
            st8(ga, pack4(z));
            st8(ga + H, pack4(r));
            st8(ga + 2 * H, pack4(n));
            st8(ga + 3 * H, pack4(q));
          }
        }
      }
    }
    __syncthreads();
  }
}

// ===========================================================================
// Two-step backward (reverse-time) scan.
//   dSeq [G, B, T, H] bf16 (or [G, B, H] with LAST_ONLY)
//   gacts [G, B, T, 4H], hs [G, B, T, H] bf16;  Wh [G, H, 3H] bf16, native:
//   its rows are already K-contiguous for carry = dGh @ Wh^T (K = 3H)
//   dGx, dGh [G, B, T, 3H] bf16 out
// LDS: dgS [2][ROWS][round32(3H) + 8] bf16 = dGh of the step before, the
// B operand; columns [3H, ..) are zeroed once and never written. 3H is a
// multiple of 16, not always of 32: the upper half of the last k-step
// then meets that zero pad, and its Wh chunk is loaded from a clamped
// address and selected to zero.
// The carry never passes through bf16: the MFMA accumulator of step t is
// joined in registers by dh_{t+1} ⊙ z_{t+1} (dhz, kept per lane across
// the step in fp32: up to 4 tiles x ROWS/16 blocks x 4 units) and by
// dSeq_t, and the same lane does step t's gate backward, stores dGx / dGh
// and writes dGh into the other dgS buffer. The loads of step t
// {gacts_t, hs_{t-1}, dSeq_t} are issued above its K loop and untouched
// until the epilogue. With LAST_ONLY dhz starts as dh_last and the loop
// loads no dSeq.
// ===========================================================================
template <int ROWS, bool LAST_ONLY>
__global__ __launch_bounds__(256) void gru_seq_bwd_big_kernel(
    const bf16* __restrict__ dSeq, const bf16* __restrict__ gacts,
    const bf16* __restrict__ hs, const bf16* __restrict__ Wh,
    bf16* __restrict__ dGx, bf16* __restrict__ dGh, int B, int T, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int H3 = 3 * H, H4 = 4 * H;
  const int LDG = ((H3 + 31) & ~31) + 8;
  bf16* dgS = reinterpret_cast<bf16*>(smem);  // [2][ROWS][LDG]

  const int nb = (B + ROWS - 1) / ROWS;
  const int g = blockIdx.x / nb;
  const int r0 = (blockIdx.x % nb) * ROWS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15;
  const int kslot = lane >> 4;

  const bf16* Whg = Wh + (size_t)g * H * H3;
  const bf16* gag = gacts + ((size_t)g * B + r0) * T * H4;
  const bf16* hsg = hs + ((size_t)g * B + r0) * T * H;
  const bf16* dSg = LAST_ONLY ? dSeq + ((size_t)g * B + r0) * H
                              : dSeq + ((size_t)g * B + r0) * T * H;
  bf16* dGxg = dGx + ((size_t)g * B + r0) * T * H3;
  bf16* dGhg = dGh + ((size_t)g * B + r0) * T * H3;
  const int rows_here = min(ROWS, B - r0);

  for (int i = tid; i < 2 * ROWS * LDG / 8; i += 256) {
    bf16x8 zero = {};
    *reinterpret_cast<bf16x8*>(&dgS[i * 8]) = zero;
  }

  constexpr int FM = ROWS / 16;
  constexpr int TS = 4;  // unit tiles per wave: H <= 256
  const int NT = H / 16;
  int rowc[FM];
  #pragma unroll
  for (int fm = 0; fm < FM; ++fm) rowc[fm] = min(fm * 16 + l15, rows_here - 1);

  float dhz[TS][FM][4];
  #pragma unroll
  for (int s = 0; s < TS; ++s) {
    // tiles past NT are never worked on; their clamped unit keeps the
    // seed load inside the row
    const int unit = min(wid + 4 * s, NT - 1) * 16 + kslot * 4;
    #pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      if (LAST_ONLY) {
        unpack4(ld8(dSg + (size_t)rowc[fm] * H + unit), dhz[s][fm]);
      } else {
        #pragma unroll
        for (int j = 0; j < 4; ++j) dhz[s][fm][j] = 0.f;
      }
    }
  }
  __syncthreads();

  for (int t = T - 1; t >= 0; --t) {
    const int cur = (T - 1 - t) & 1;
    const bf16* dc = dgS + (size_t)cur * ROWS * LDG;
    bf16* dn = dgS + (size_t)(cur ^ 1) * ROWS * LDG;
    const int kend = t == T - 1 ? 0 : H3;  // no carry enters the last step
    const int tp = max(t - 1, 0);          // hs_{t-1}; taken as 0 at t = 0
    #pragma unroll
    for (int s = 0; s < TS; ++s) {
      const int u = wid + 4 * s;
      if (u < NT) {  // wave-uniform
        const int unit = u * 16 + kslot * 4;
        uint2 gz[FM], gr[FM], gn[FM], gq[FM], hv[FM], dv[FM];
        #pragma unroll
        for (int fm = 0; fm < FM; ++fm) {
          const size_t rT = (size_t)rowc[fm] * T;
          const bf16* ga = gag + (rT + t) * H4 + unit;
          gz[fm] = ld8(ga);
          gr[fm] = ld8(ga + H);
          gn[fm] = ld8(ga + 2 * H);
          gq[fm] = ld8(ga + 3 * H);
          hv[fm] = ld8(hsg + (rT + tp) * H + unit);
          if (!LAST_ONLY) dv[fm] = ld8(dSg + (rT + t) * H + unit);
        }

        f32x4 acc[FM] = {};
        const bf16* wrow = Whg + (size_t)(u * 16 + l15) * H3;
        const bf16* db = dc + l15 * LDG + kslot * 8;
        for (int kk = 0; kk < kend; kk += 32) {
          const int k = kk + kslot * 8;
          bf16x8 a = *reinterpret_cast<const bf16x8*>(wrow + min(k, H3 - 8));
          const bf16x8 zero = {};
          a = k < H3 ? a : zero;
          #pragma unroll
          for (int fm = 0; fm < FM; ++fm) {
            bf16x8 b =
                *reinterpret_cast<const bf16x8*>(db + fm * 16 * LDG + kk);
            acc[fm] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[fm], 0, 0, 0);
          }
        }

        #pragma unroll
        for (int fm = 0; fm < FM; ++fm) {
          const int row = fm * 16 + l15;
          float z[4], r[4], n[4], q[4], hp[4], ds[4];
          float daz[4], dar[4], dan[4], dq[4];
          unpack4(gz[fm], z);
          unpack4(gr[fm], r);
          unpack4(gn[fm], n);
          unpack4(gq[fm], q);
          unpack4(hv[fm], hp);
          if (!LAST_ONLY) unpack4(dv[fm], ds);
          #pragma unroll
          for (int j = 0; j < 4; ++j) {
            float dh = acc[fm][j] + dhz[s][fm][j];
            if (!LAST_ONLY) dh += ds[j];
            const float hprev = t > 0 ? hp[j] : 0.f;
            dan[j] = dh * (1.f - z[j]) * (1.f - n[j] * n[j]);
            daz[j] = dh * (hprev - n[j]) * z[j] * (1.f - z[j]);
            dar[j] = dan[j] * q[j] * r[j] * (1.f - r[j]);
            dq[j] = dan[j] * r[j];
            dhz[s][fm][j] = dh * z[j];
          }
          const uint2 pz = pack4(daz), pr = pack4(dar), pn = pack4(dan),
                      pq = pack4(dq);
          bf16* dg = dn + row * LDG + unit;
          st8(dg, pz);
          st8(dg + H, pr);
          st8(dg + 2 * H, pq);
          if (row < rows_here) {
            const size_t o = ((size_t)row * T + t) * H3 + unit;
            st8(dGxg + o, pz);
            st8(dGxg + o + H, pr);
            st8(dGxg + o + 2 * H, pn);
            st8(dGhg + o, pz);
            st8(dGhg + o + H, pr);
            st8(dGhg + o + 2 * H, pq);
          }
        }
      }
    }
    __syncthreads();
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// Host side: scan_plan.h's plan_gru() decides row tile, LDS bytes and grid;
// the launchers launch the plan they get and record it.
// ---------------------------------------------------------------------------
using gordo_lstm::GruPlan;
using gordo_lstm::GruRequest;
using gordo_lstm::ScanEnv;

thread_local GruPlan g_last_gru;

// (family, rows, has_dx, last_only, lds_bytes, blocks); family "" before
// any launch
std::tuple<std::string, int, int, int, int64_t, int> last_gru_launch() {
  const GruPlan& l = g_last_gru;
  return {l.rows ? l.family_name() : "", l.rows, l.has_dx, l.last_only,
          (int64_t)l.lds_bytes, l.blocks};
}

// (family, rows, has_dx, last_only, lds_bytes, blocks, error): the plan of
// a request, without touching the GPU
std::tuple<std::string, int, int, int, int64_t, int, std::string> gru_plan(
    bool fwd, int G, int B, int T, int H, int F, bool has_dx,
    bool last_only) {
  GruPlan p = gordo_lstm::plan_gru({fwd, G, B, T, H, F, has_dx, last_only},
                                   ScanEnv::read());
  return {p.ok() ? p.family_name() : "", p.rows, p.has_dx, p.last_only,
          (int64_t)p.lds_bytes, p.blocks, p.error};
}

inline GruPlan planned(const GruRequest& q) {
  GruPlan p = gordo_lstm::plan_gru(q, ScanEnv::read());
  TORCH_CHECK(p.ok(), p.error);
  return p;
}

template <class Fn>
inline void pick_tile(int rows, Fn&& f) {
  if (rows == 16) f(std::integral_constant<int, 16>{});
  else if (rows == 32) f(std::integral_constant<int, 32>{});
  else if (rows == 64) f(std::integral_constant<int, 64>{});
  else TORCH_CHECK(false, "no GRU scan kernel instantiated for rows ", rows);
}
template <class Fn>
inline void pick(bool v, Fn&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

template <class Kernel, class... Args>
inline void launch(Kernel kernel, const GruPlan& p, Args... args) {
  g_last_gru = p;
  hipLaunchKernelGGL(kernel, dim3(p.blocks), dim3(256), p.lds_bytes,
                     at::cuda::getCurrentCUDAStream().stream(), args...);
}

inline torch::Tensor as_bf16(const torch::Tensor& t) {
  return t.to(torch::kBFloat16).contiguous();
}
inline const bf16* rd(const torch::Tensor& t) {
  return (const bf16*)t.data_ptr();
}
inline bf16* wr(const torch::Tensor& t) { return (bf16*)t.data_ptr(); }

inline void check_shape(const torch::Tensor& t, std::vector<int64_t> shape,
                        const char* what) {
  TORCH_CHECK(t.is_cuda() && t.sizes().vec() == shape, what,
              " has the wrong shape or device for this GRU scan");
}

// mx [G,B,T,3H] = x @ Wx + b[0]; Wh [G,H,3H]; bh [G,3H] = b[1]
// -> {hs, gacts} ({hs} without store_aux): the two-step forward scan alone
std::vector<torch::Tensor> gru_seq_fwd_big(torch::Tensor mx, torch::Tensor Wh,
                                           torch::Tensor bh, bool store_aux) {
  TORCH_CHECK(mx.is_cuda() && mx.dim() == 4, "mx must be [G,B,T,3H] on GPU");
  TORCH_CHECK(Wh.dim() == 3, "Wh must be [G,H,3H]");
  auto mc = as_bf16(mx);
  const int G = mc.size(0), B = mc.size(1), T = mc.size(2);
  const int H = Wh.size(1), H3 = 3 * H;
  check_shape(mx, {G, B, T, H3}, "mx");
  check_shape(Wh, {G, H, H3}, "Wh");
  check_shape(bh, {G, H3}, "bh");
  const GruPlan p = planned({true, G, B, T, H, 0, false, false, true});
  // K-contiguous rows with a zero K tail up to the MFMA K step
  const int Kp = gordo_lstm::round32(H);
  auto WhT = torch::zeros({G, H3, Kp}, mc.options());
  WhT.narrow(2, 0, H).copy_(Wh.to(torch::kBFloat16).transpose(1, 2));
  auto bf = bh.to(torch::kFloat32).contiguous();
  auto hs = torch::empty({G, B, T, H}, mc.options());
  auto gacts = store_aux ? torch::empty({G, B, T, 4 * H}, mc.options())
                         : torch::empty({1}, mc.options());
  pick_tile(p.rows, [&](auto R) {
    pick(store_aux, [&](auto AUX) {
      launch(gru_seq_fwd_big_kernel<decltype(R)::value, decltype(AUX)::value>,
             p, rd(mc), rd(WhT), bf.data_ptr<float>(), wr(hs), wr(gacts), B,
             T, H, Kp);
    });
  });
  if (store_aux) return {hs, gacts};
  return {hs};
}

// dSeq [G,B,T,H] (or [G,B,H] with last_only); gacts [G,B,T,4H];
// hs [G,B,T,H]; Wh [G,H,3H] -> {dGx, dGh}: the two-step reverse scan alone
std::vector<torch::Tensor> gru_seq_bwd_big(torch::Tensor dSeq,
                                           torch::Tensor gacts,
                                           torch::Tensor hs, torch::Tensor Wh,
                                           bool last_only) {
  TORCH_CHECK(gacts.is_cuda() && gacts.dim() == 4,
              "gacts must be [G,B,T,4H] on GPU");
  auto gc = as_bf16(gacts);
  const int G = gc.size(0), B = gc.size(1), T = gc.size(2), H4 = gc.size(3);
  const int H = H4 / 4, H3 = 3 * H;
  TORCH_CHECK(H4 == 4 * H, "gacts must be [G,B,T,4H]");
  check_shape(hs, {G, B, T, H}, "hs");
  check_shape(Wh, {G, H, H3}, "Wh");
  if (last_only) check_shape(dSeq, {G, B, H}, "dSeq");
  else check_shape(dSeq, {G, B, T, H}, "dSeq");
  const GruPlan p = planned({false, G, B, T, H, 0, false, last_only, true});
  auto dc = as_bf16(dSeq), hc = as_bf16(hs), Whc = as_bf16(Wh);
  auto dGx = torch::empty({G, B, T, H3}, gc.options());
  auto dGh = torch::empty({G, B, T, H3}, gc.options());
  pick_tile(p.rows, [&](auto R) {
    pick(last_only, [&](auto LO) {
      launch(gru_seq_bwd_big_kernel<decltype(R)::value, decltype(LO)::value>,
             p, rd(dc), rd(gc), rd(hc), rd(Whc), wr(dGx), wr(dGh), B, T, H);
    });
  });
  return {dGx, dGh};
}

// xseq [G,B,T,F]; Wx [G,F,3H]; Wh [G,H,3H]; bias [G,2,3H] -> {hs, gacts}
// ({hs} without store_aux)
std::vector<torch::Tensor> gru_seq_fwd(torch::Tensor xseq, torch::Tensor Wx,
                                       torch::Tensor Wh, torch::Tensor bias,
                                       bool store_aux) {
  TORCH_CHECK(xseq.is_cuda() && xseq.dim() == 4,
              "xseq must be [G,B,T,F] on GPU");
  TORCH_CHECK(Wh.dim() == 3, "Wh must be [G,H,3H]");
  auto xc = as_bf16(xseq);
  const int G = xc.size(0), B = xc.size(1), T = xc.size(2), F = xc.size(3);
  const int H = Wh.size(1), H4 = 4 * H;
  check_shape(Wh, {G, H, 3 * H}, "Wh");
  check_shape(Wx, {G, F, 3 * H}, "Wx");
  check_shape(bias, {G, 2, 3 * H}, "bias");
  const GruPlan p = planned({true, G, B, T, H, F, false, false});
  if (p.big()) {  // two-step: one GEMM over all B * T rows, then the scan
    auto mx = gordo_gemm::linear_fwd(xc.view({G, B * T, F}), Wx,
                                     bias.select(1, 0));
    return gru_seq_fwd_big(mx.view({G, B, T, 3 * H}), Wh, bias.select(1, 1),
                           store_aux);
  }
  auto Whc = Wh.to(torch::kBFloat16), Wxc = Wx.to(torch::kBFloat16);
  // [G, Kc, 4H] with the zero blocks of n_x / n_h, then K-contiguous
  auto W4 = torch::zeros({G, H + F, H4}, xc.options());
  W4.narrow(1, 0, H).narrow(2, 0, 2 * H).copy_(Whc.narrow(2, 0, 2 * H));
  W4.narrow(1, H, F).narrow(2, 0, 3 * H).copy_(Wxc);
  W4.narrow(1, 0, H).narrow(2, 3 * H, H).copy_(Whc.narrow(2, 2 * H, H));
  auto WcatT = W4.transpose(1, 2).contiguous();
  auto bf = bias.to(torch::kFloat32);
  auto b0 = bf.select(1, 0), b1 = bf.select(1, 1);
  auto bias4 = torch::cat({(b0 + b1).narrow(1, 0, 2 * H),
                           b0.narrow(1, 2 * H, H), b1.narrow(1, 2 * H, H)},
                          1)
                   .contiguous();
  auto hs = torch::empty({G, B, T, H}, xc.options());
  auto gacts = store_aux ? torch::empty({G, B, T, H4}, xc.options())
                         : torch::empty({1}, xc.options());
  pick_tile(p.rows, [&](auto R) {
    pick(store_aux, [&](auto AUX) {
      launch(gru_seq_fwd_kernel<decltype(R)::value, decltype(AUX)::value>, p,
             rd(xc), rd(WcatT), bias4.data_ptr<float>(), wr(hs), wr(gacts), B,
             T, H, F);
    });
  });
  if (store_aux) return {hs, gacts};
  return {hs};
}

// dSeq [G,B,T,H] (or [G,B,H] with last_only); gacts [G,B,T,4H];
// hs [G,B,T,H]; Wh [G,H,3H]; Wx [G,F,3H] or none -> {dGx, dGh[, dX]}
std::vector<torch::Tensor> gru_seq_bwd(torch::Tensor dSeq,
                                       torch::Tensor gacts, torch::Tensor hs,
                                       torch::Tensor Wh, bool last_only,
                                       c10::optional<torch::Tensor> Wx) {
  TORCH_CHECK(gacts.is_cuda() && gacts.dim() == 4,
              "gacts must be [G,B,T,4H] on GPU");
  auto gc = as_bf16(gacts);
  const int G = gc.size(0), B = gc.size(1), T = gc.size(2), H4 = gc.size(3);
  const int H = H4 / 4, H3 = 3 * H;
  TORCH_CHECK(H4 == 4 * H, "gacts must be [G,B,T,4H]");
  const bool has_dx = Wx.has_value();
  const int F = has_dx ? (int)Wx->size(1) : 0;
  check_shape(hs, {G, B, T, H}, "hs");
  check_shape(Wh, {G, H, H3}, "Wh");
  if (last_only) check_shape(dSeq, {G, B, H}, "dSeq");
  else check_shape(dSeq, {G, B, T, H}, "dSeq");
  if (has_dx) check_shape(*Wx, {G, F, H3}, "Wx");
  const GruPlan p = planned({false, G, B, T, H, F, has_dx, last_only});
  if (p.big()) {  // two-step: the scan, then dX as one GEMM
    auto out = gru_seq_bwd_big(dSeq, gacts, hs, Wh, last_only);
    if (has_dx)
      out.push_back(
          gordo_gemm::linear_bwd_data(out[0].view({G, B * T, H3}), *Wx)
              .view({G, B, T, F}));
    return out;
  }
  auto dc = as_bf16(dSeq), hc = as_bf16(hs), Whc = as_bf16(Wh);
  auto Wxc = has_dx ? as_bf16(*Wx) : torch::Tensor();
  auto dGx = torch::empty({G, B, T, H3}, gc.options());
  auto dGh = torch::empty({G, B, T, H3}, gc.options());
  auto dX = has_dx ? torch::empty({G, B, T, F}, gc.options()) : torch::Tensor();
  const int ldg = gordo_lstm::pad_ldg(H4);
  pick_tile(p.rows, [&](auto R) {
    pick(has_dx, [&](auto DX) {
      pick(last_only, [&](auto LO) {
        launch(gru_seq_bwd_kernel<decltype(R)::value, decltype(DX)::value,
                                  decltype(LO)::value>,
               p, rd(dc), rd(gc), rd(hc), rd(Whc),
               has_dx ? rd(Wxc) : nullptr, wr(dGx), wr(dGh),
               has_dx ? wr(dX) : nullptr, B, T, H, F, ldg);
      });
    });
  });
  if (has_dx) return {dGx, dGh, dX};
  return {dGx, dGh};
}

}  // namespace gordo_gru
