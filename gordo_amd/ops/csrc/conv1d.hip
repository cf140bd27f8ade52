// Grouped Conv1D for MI355X (gfx950): Keras Conv1D with strides = 1,
// groups = 1, channels last, "same" or "causal" padding, for G models at
// once. bf16 tensors, fp32 accumulation on mfma_f32_16x16x32_bf16.
//
//   y[g,b,t,:] = act( sum_{j<k} x[g,b, t + j*d - left, :] @ W[g,j] + bias[g] )
//
// with rows outside [0, T) zero. Three kernels (docs/kernels.md,
// "Grouped Conv1D"):
//
//   conv1d_tile_kernel<ROWS, MODE, ACT>
//     MODE 0, the forward: x [G,B,T,Cin] -> y [G,B,T,Cout], bias and
//     activation in the epilogue.
//     MODE 1, bwd-data: dZ [G,B,T,Cout] -> dX [G,B,T,Cin]: the same tile
//     machinery with the tap offsets negated and the weight panel read in
//     its other orientation.
//     A work item is (model, window, ROWS-row time tile): a tile never
//     crosses a window, so the padding zeros are ROWS OF ZEROS in the LDS
//     image, not masks in the MFMA loop. The image [ROWS + (k-1)*d][C] is
//     read from global memory once per item and every tap's A fragments
//     come from it at a shifted row. A workgroup owns one model and a
//     contiguous range of items: the weight panels are staged once
//     (transposed, [n][c]), the image is double-buffered with one barrier
//     per item, and the output leaves as 16-byte stores through an LDS
//     staging tile.
//   conv1d_wgrad_kernel<KF2, NF2, TG>
//     dW[g,j,ci,co] = sum_m x[m + j*d - left, ci] * dZ[m, co], db = colsum
//     dZ. Window-aligned 32-row steps; the x image (with halo, zero rows
//     at the window edges) and the dZ image are staged row-major once per
//     step and both MFMA operands are read column-wise with
//     ds_read_b64_tr_b16; tap j reads the x image j*d rows further down.
//
// The geometry (8 <= C <= 128 in multiples of 8, k <= 8, (k-1)*d <= 64,
// T < 2^17) and every launch parameter come from conv_plan.h.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "conv_plan.h"

#define DEV_INLINE __device__ __forceinline__

namespace gordo_conv {

// device code of this file is built without packed fp32 instructions
// (v_pk_{add,mul,fma}_f32), like gru_seq.hip
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// activation codes and formulas of grouped_linear_fwd (gordo_kernels.hip:
// act_apply / fast_tanhf), with the code as a template parameter
constexpr int ACT_LINEAR = 0, ACT_TANH = 1, ACT_RELU = 2, ACT_SIGMOID = 3;

template <int ACT>
DEV_INLINE float act_apply(float z) {
  if (ACT == ACT_TANH) {
    float e = __expf(2.f * z);
    return 1.f - 2.f / (e + 1.f);  // saturates to 1 when e overflows to inf
  }
  if (ACT == ACT_RELU) return z > 0.f ? z : 0.f;
  if (ACT == ACT_SIGMOID) return 1.f / (1.f + __expf(-z));
  return z;
}

constexpr int IMG_IT_MAX = 8;  // 16-byte image chunks per thread, at most

// ===========================================================================
// Forward (MODE 0) and bwd-data (MODE 1).
//   X    [G, B, T, Ck]      bf16   Ck: contracted channels
//   W    [G, k, Cin, Cout]  bf16   (Ck, Cn) = (Cin, Cout) forward,
//                                  (Cout, Cin) bwd-data
//   bias [G, Cn]            f32    forward only
//   Y    [G, B, T, Cn]      bf16
// Image row i of an item at (b, t0) is source row t0 - base_off + i; output
// row r and tap j read image row r + j*d (bwd-data: r + (k-1-j)*d against
// the mirrored base_off).
// LDS: Wt [slots][CNR][LDK] | img [2][IR][LDK] | outS [2][ROWS][Cn+8], bf16;
// LDK = round32(Ck) + 8, CNR = round16(Cn), IR = ROWS + (k-1)*d, slots = k
// (resident) or 2 (ring, restaged per item).
// ===========================================================================
template <int ROWS, int MODE, int ACT>
__global__ __launch_bounds__(256) void conv1d_tile_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ W,
    const float* __restrict__ bias, bf16* __restrict__ Y, int B, int T,
    int Ck, int Cn, int k, int d, int base_off, int resident, int chunks,
    int ipc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int RF = ROWS / 16;
  const int IR = ROWS + (k - 1) * d;
  const int KP = (Ck + 31) & ~31;
  const int LDK = KP + 8;
  const int CNR = (Cn + 15) & ~15;
  const int LDO = Cn + 8;
  bf16* Wt = reinterpret_cast<bf16*>(smem);
  bf16* img = Wt + (size_t)(resident ? k : 2) * CNR * LDK;
  bf16* outS = img + (size_t)2 * IR * LDK;

  const int g = blockIdx.x / chunks;
  const int tiles = (T + ROWS - 1) / ROWS;
  const int items = B * tiles;
  const int it_begin = (blockIdx.x % chunks) * ipc;
  const int it_end = it_begin + ipc < items ? it_begin + ipc : items;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // wave-uniform by construction; readfirstlane keeps the per-wave
  // choices below in scalar registers and scalar branches
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15;
  const int kslot = lane >> 4;
  const u32x4 zero = {0u, 0u, 0u, 0u};

  // ---- weight panel of tap j -> Wt[slot], transposed to [n][c] ----
  // rows n >= Cn and the K tail [Ck, KP) are zero
  const bf16* Wg = W + (size_t)g * k * Ck * Cn;
  const int CW = KP / 8;
  auto stage_tap = [&](int j, int slot) {
    bf16* dst = Wt + (size_t)slot * CNR * LDK;
    const bf16* src = Wg + (size_t)j * Ck * Cn;
    for (int i = tid; i < CNR * CW; i += 256) {
      // forward gathers a column of W[j] ([c][n]): n runs fastest over
      // the lanes; bwd-data copies 16-byte chunks of its rows ([n][c])
      const int n = MODE == 0 ? i % CNR : i / CW;
      const int c = (MODE == 0 ? i / CNR : i % CW) * 8;
      u32x4 v = zero;
      if (n < Cn && c < Ck) {
        if (MODE == 0) {
          bf16 t[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) t[e] = src[(size_t)(c + e) * Cn + n];
          v = *reinterpret_cast<const u32x4*>(t);
        } else {
          v = *reinterpret_cast<const u32x4*>(src + (size_t)n * Ck + c);
        }
      }
      *reinterpret_cast<u32x4*>(dst + n * LDK + c) = v;
    }
  };

  // ---- image chunk map (constant over the items) ----
  const int CH = Ck / 8;
  const int total = IR * CH;
  const int nit = (total + 255) / 256;  // <= IMG_IT_MAX, wave-uniform
  int i_row[IMG_IT_MAX], i_col[IMG_IT_MAX];
#pragma unroll
  for (int i = 0; i < IMG_IT_MAX; ++i) {
    // chunks past the image repeat its last one (same address, same value)
    const int idx = tid + 256 * i < total ? tid + 256 * i : total - 1;
    i_row[i] = idx / CH;
    i_col[i] = (idx % CH) * 8;
  }
  u32x4 reg[IMG_IT_MAX];
  bool ok[IMG_IT_MAX];

  // IMG_LOAD: clamped addresses, never a branch around a load within a
  // wave; the zero-select happens at the LDS write. An item past the
  // chunk's last reloads that one (its image is never read).
  auto img_load = [&](int it) {
    const int itc = it < it_end ? it : it_end - 1;
    const int b = itc / tiles, t0 = (itc % tiles) * ROWS;
    const bf16* xb = X + ((size_t)g * B + b) * T * Ck;
    const int s0 = t0 - base_off;
#pragma unroll
    for (int i = 0; i < IMG_IT_MAX; ++i) {
      if (i < nit) {
        const int s = s0 + i_row[i];
        ok[i] = s >= 0 && s < T;
        const int sc = s < 0 ? 0 : (s < T ? s : T - 1);
        reg[i] = *reinterpret_cast<const u32x4*>(xb + (size_t)sc * Ck +
                                                 i_col[i]);
      }
    }
  };
  auto img_write = [&](bf16* buf) {
#pragma unroll
    for (int i = 0; i < IMG_IT_MAX; ++i)
      if (i < nit)
        *reinterpret_cast<u32x4*>(buf + i_row[i] * LDK + i_col[i]) =
            ok[i] ? reg[i] : zero;
  };

  // the K tail of both image buffers is zero for the whole launch
  {
    const int tailc = (KP - Ck) / 8;
    for (int i = tid; i < 2 * IR * tailc; i += 256)
      *reinterpret_cast<u32x4*>(img + (i / tailc) * LDK + Ck +
                                (i % tailc) * 8) = zero;
  }

  // wave w owns the 16-column fragments w and w + 4 of every row fragment
  float bv[2] = {0.f, 0.f};
  if (MODE == 0) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int col = (wid + 4 * c) * 16 + l15;
      if (col < Cn) bv[c] = bias[(size_t)g * Cn + col];
    }
  }

  if (resident)
    for (int j = 0; j < k; ++j) stage_tap(j, j);
  img_load(it_begin);
  img_write(img);
  __syncthreads();

  int cur = 0;
  for (int it = it_begin; it < it_end; ++it) {
    const bf16* ib = img + (size_t)cur * IR * LDK;
    img_load(it + 1);
    __builtin_amdgcn_sched_barrier(0);

    f32x4 acc[RF][2] = {};
    for (int j = 0; j < k; ++j) {
      const bf16* Wj = Wt + (size_t)(resident ? j : (j & 1)) * CNR * LDK;
      if (!resident) {
        // two-tap ring: tap j + 1 is written while other waves still
        // multiply tap j; the barrier before tap j + 2 reuses slot j & 1
        // is the one after staging tap j + 1
        stage_tap(j, j & 1);
        __syncthreads();
      }
      const int joff = (MODE == 0 ? j : k - 1 - j) * d;
      for (int ks = 0; ks < KP; ks += 32) {
        bf16x8 bfr[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
          if ((wid + 4 * c) * 16 < Cn)
            bfr[c] = *reinterpret_cast<const bf16x8*>(
                Wj + ((wid + 4 * c) * 16 + l15) * LDK + ks + kslot * 8);
#pragma unroll
        for (int rf = 0; rf < RF; ++rf) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(
              ib + (rf * 16 + l15 + joff) * LDK + ks + kslot * 8);
#pragma unroll
          for (int c = 0; c < 2; ++c)
            if ((wid + 4 * c) * 16 < Cn)
              acc[rf][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a, bfr[c], acc[rf][c], 0, 0, 0);
        }
      }
    }

    // ---- epilogue: fp32 bias, activation, ONE rounding to bf16 ----
    bf16* ob = outS + (size_t)cur * ROWS * LDO;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int col = (wid + 4 * c) * 16 + l15;
      if (col < Cn) {
#pragma unroll
        for (int rf = 0; rf < RF; ++rf)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            ob[(rf * 16 + kslot * 4 + r) * LDO + col] =
                __float2bfloat16(act_apply<ACT>(acc[rf][c][r] + bv[c]));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    img_write(img + (size_t)(cur ^ 1) * IR * LDK);
    __syncthreads();

    // 16-byte stores from the staging tile, masked by row. outS[cur] is
    // written again two items on, behind the next item's barrier.
    {
      const int b = it / tiles, t0 = (it % tiles) * ROWS;
      bf16* yb = Y + (((size_t)g * B + b) * T + t0) * Cn;
      const int OC = Cn / 8;
      for (int i = tid; i < ROWS * OC; i += 256) {
        const int row = i / OC, c = (i % OC) * 8;
        if (t0 + row < T)
          *reinterpret_cast<u32x4*>(yb + (size_t)row * Cn + c) =
              *reinterpret_cast<const u32x4*>(ob + row * LDO + c);
      }
    }
    cur ^= 1;
  }
}

// ===========================================================================
// Weight-grad.
//   X [G,B,T,Cin], dZ [G,B,T,Cout] bf16 -> dW [G,k,Cin,Cout], db [G,Cout] f32
// grid (G, chunks of whole windows, tap groups). The image addressing is
// that of wgrad_pipe.hip: row stride cols*2 + 32 bytes with cols a
// multiple of 32 (an ODD multiple of 32 B), transposed 8-byte reads.
// ===========================================================================
constexpr int MS = WGRAD_ROWS;

constexpr __host__ __device__ int img_stride(int cols) { return cols * 2 + 32; }
// byte address lane `lane` supplies to transposed read `rd` (0/1) of the
// 16 columns of fragment `frag` (wgrad_pipe.hip, img_tr_off)
constexpr __host__ __device__ int img_tr_off(int stride, int lane, int frag,
                                             int rd) {
  const int g = (lane >> 4) & 3, q = (lane >> 2) & 3, p = lane & 3;
  return (16 * rd + 4 * g + q) * stride + (frag * 16 + 4 * p) * 2;
}
// a row shift moves every lane of a read by the same multiple of the
// stride: alignment and the bank pattern are those of shift 0
constexpr bool img_tr_reads_ok(int cols, int shift) {
  const int stride = img_stride(cols);
  for (int frag = 0; frag < cols / 16; ++frag)
    for (int rd = 0; rd < 2; ++rd)
      for (int half = 0; half < 2; ++half) {
        int used[64] = {};
        for (int l = 0; l < 32; ++l) {
          const int off =
              img_tr_off(stride, half * 32 + l, frag, rd) + shift * stride;
          if (off % 8 != 0) return false;
          for (int w = 0; w < 2; ++w)
            if (used[(off / 4 + w) % 64]++) return false;
        }
      }
  return true;
}
static_assert(img_tr_reads_ok(64, 0) && img_tr_reads_ok(128, 0) &&
                  img_tr_reads_ok(64, 1) && img_tr_reads_ok(128, 3) &&
                  img_tr_reads_ok(64, 16) && img_tr_reads_ok(128, 64),
              "transposed reads must be aligned and conflict-free");

DEV_INLINE bf16x8 tr_operand(const char* img, int off, int stride) {
  typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
  i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(img + off));
  i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_i16x4*)(img + off + 16 * stride));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// KF2 / NF2: 16x16 fragments per wave along Cin / Cout (2 x 2 waves);
// TG: taps whose accumulators one workgroup holds (TG * KF2 * NF2 = 32
// fragments = 128 accumulator registers). Padding fragments multiply
// zero-filled LDS.
template <int KF2, int NF2, int TG>
__global__ __launch_bounds__(256) void conv1d_wgrad_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ dZ,
    float* __restrict__ dW, float* __restrict__ db, int B, int T, int Cin,
    int Cout, int k, int d, int left, int wpc) {
  constexpr int KC = KF2 * 32, NC = NF2 * 32;
  constexpr int SA = img_stride(KC), SZ = img_stride(NC);
  constexpr int A_CH = KC / 8, Z_CH = NC / 8;
  constexpr int Z_IT = MS * Z_CH / 256;
  constexpr int X_IT_MAX = ((MS + MAX_HALO) * A_CH + 255) / 256;
  static_assert(MS * Z_CH % 256 == 0, "chunk map");
  extern __shared__ __attribute__((aligned(16))) char sm[];

  const int g = blockIdx.x;
  const int j0 = blockIdx.z * TG;
  const int nt = k - j0 < TG ? k - j0 : TG;  // taps of this group
  const int XR = MS + (nt - 1) * d;          // x image rows
  const int A_BYTES = XR * SA, BUF = A_BYTES + MS * SZ;
  const int nx = (XR * A_CH + 255) / 256;    // <= X_IT_MAX, uniform

  const int b_begin = blockIdx.y * wpc;
  const int b_end = b_begin + wpc < B ? b_begin + wpc : B;
  const int tiles = (T + MS - 1) / MS;
  const int nsteps = (b_end - b_begin) * tiles;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wid & 1, wn = wid >> 1;

  u32x4 x_reg[X_IT_MAX], z_reg[Z_IT];
  bool x_ok[X_IT_MAX], z_ok[Z_IT];

  // STAGE_LOAD of step s = (window, 32-row tile): clamped addresses, the
  // zero-select at the LDS write. x image row i is source row
  // t0 - left + j0*d + i: rows outside the window are ZERO rows, so no
  // (tap, row) pair needs a mask in the MFMA loop.
  auto stage_load = [&](int s) {
    const bool live = s < nsteps;
    const int sc = live ? s : nsteps - 1;
    const int b = b_begin + sc / tiles, t0 = (sc % tiles) * MS;
    const bf16* xb = X + ((size_t)g * B + b) * T * Cin;
    const bf16* zb = dZ + ((size_t)g * B + b) * T * Cout;
    const int xs0 = t0 - left + j0 * d;
#pragma unroll
    for (int i = 0; i < X_IT_MAX; ++i) {
      if (i < nx) {
        const int idx = tid + 256 * i;
        const int row = idx / A_CH, c = (idx % A_CH) * 8;
        const int src = xs0 + row;
        x_ok[i] = live && src >= 0 && src < T && c < Cin;
        const int r = src < 0 ? 0 : (src < T ? src : T - 1);
        x_reg[i] = *reinterpret_cast<const u32x4*>(xb + (size_t)r * Cin +
                                                   (c < Cin ? c : 0));
      }
    }
#pragma unroll
    for (int i = 0; i < Z_IT; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / Z_CH, c = (idx % Z_CH) * 8;
      const int src = t0 + row;
      z_ok[i] = live && src < T && c < Cout;
      z_reg[i] = *reinterpret_cast<const u32x4*>(
          zb + (size_t)(src < T ? src : T - 1) * Cout + (c < Cout ? c : 0));
    }
  };
  auto stage_write = [&](char* buf) {
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < X_IT_MAX; ++i) {
      const int idx = tid + 256 * i;
      const int row = idx / A_CH;
      if (i < nx && row < XR)
        *reinterpret_cast<u32x4*>(buf + row * SA + (idx % A_CH) * 16) =
            x_ok[i] ? x_reg[i] : zero;
    }
#pragma unroll
    for (int i = 0; i < Z_IT; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<u32x4*>(buf + A_BYTES + (idx / Z_CH) * SZ +
                                (idx % Z_CH) * 16) =
          z_ok[i] ? z_reg[i] : zero;
    }
  };

  f32x4 acc[TG][KF2][NF2] = {};
  f32x4 acc_db[NF2 / 2] = {};
  const short one_bf16 = 0x3F80;
  const bf16x8 ones = {one_bf16, one_bf16, one_bf16, one_bf16,
                       one_bf16, one_bf16, one_bf16, one_bf16};
  const bool do_db = blockIdx.z == 0;  // block-uniform

  const int a_tr0 = img_tr_off(SA, lane, wk * KF2, 0);
  const int z_tr0 = A_BYTES + img_tr_off(SZ, lane, wn * NF2, 0);

  stage_load(0);
  stage_write(sm);
  __syncthreads();

  int cur = 0;
  for (int s = 0; s < nsteps; ++s) {
    const char* rbuf = sm + cur * BUF;
    // the last trip loads clamped rows it then writes as zeros
    stage_load(s + 1);
    __builtin_amdgcn_sched_barrier(0);

    bf16x8 bz[NF2];
#pragma unroll
    for (int j = 0; j < NF2; ++j) bz[j] = tr_operand(rbuf, z_tr0 + j * 32, SZ);
#pragma unroll
    for (int jj = 0; jj < TG; ++jj) {
      if (jj < nt) {
#pragma unroll
        for (int i = 0; i < KF2; ++i) {
          // tap j0 + jj: the same image, jj*d rows further down
          const bf16x8 a =
              tr_operand(rbuf, a_tr0 + i * 32 + jj * d * SA, SA);
#pragma unroll
          for (int j = 0; j < NF2; ++j)
            acc[jj][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, bz[j], acc[jj][i][j], 0, 0, 0);
        }
      }
    }
    // bias-grad: wave wk sums its half of the wave's n-fragments
    if (do_db) {
#pragma unroll
      for (int j = 0; j < NF2; ++j)
        if ((j >= NF2 / 2) == (wk == 1))
          acc_db[j % (NF2 / 2)] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              ones, bz[j], acc_db[j % (NF2 / 2)], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    stage_write(sm + (cur ^ 1) * BUF);
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: plain stores from one chunk, fp32 atomics from more ----
  const bool single_chunk = gridDim.y == 1;
  const int l15 = lane & 15, rq = (lane >> 4) * 4;
#pragma unroll
  for (int j = 0; j < NF2; ++j) {
    const int col = (wn * NF2 + j) * 16 + l15;
    if (col >= Cout) continue;
    if (do_db && (j >= NF2 / 2) == (wk == 1) && rq == 0) {
      // all 16 rows of the ones-product hold the column sum; row 0
      float* dst = &db[(size_t)g * Cout + col];
      if (single_chunk) *dst = acc_db[j % (NF2 / 2)][0];
      else atomicAdd(dst, acc_db[j % (NF2 / 2)][0]);
    }
#pragma unroll
    for (int jj = 0; jj < TG; ++jj) {
      if (jj >= nt) continue;
      float* Wj = dW + ((size_t)g * k + j0 + jj) * Cin * Cout;
#pragma unroll
      for (int i = 0; i < KF2; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = (wk * KF2 + i) * 16 + rq + r;
          if (row >= Cin) continue;
          if (single_chunk) Wj[(size_t)row * Cout + col] = acc[jj][i][j][r];
          else atomicAdd(&Wj[(size_t)row * Cout + col], acc[jj][i][j][r]);
        }
      }
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// Host side: conv_plan.h's plan_conv1d() decides; the launchers launch the
// plan they get and keep it as the per-thread launch record.
// ---------------------------------------------------------------------------
thread_local ConvPlan g_last_conv;

using PlanTuple =
    std::tuple<std::string, int, bool, int64_t, int, int, std::string>;

inline PlanTuple plan_tuple(const ConvPlan& p, bool launched) {
  return {launched ? p.family_name() : "", p.rows, p.taps_resident,
          (int64_t)p.lds_bytes, p.blocks, p.chunks, p.error};
}

// (family, rows, taps_resident, lds_bytes, blocks, chunks, error): the plan
// of a request, without touching the GPU
PlanTuple conv1d_plan(const std::string& entry, int G, int B, int T, int Cin,
                      int Cout, int k, int d, const std::string& padding) {
  ConvPlan p = plan_conv1d(entry_code(entry), G, B, T, Cin, Cout, k, d,
                           padding);
  return plan_tuple(p, p.ok());
}

// the same tuple for this thread's last launch; family "" before any
PlanTuple last_conv1d_launch() {
  return plan_tuple(g_last_conv, g_last_conv.rows > 0);
}

inline ConvPlan planned(ConvEntry entry, int G, int B, int T, int Cin,
                        int Cout, int k, int d, const std::string& padding) {
  ConvPlan p = plan_conv1d(entry, G, B, T, Cin, Cout, k, d, padding);
  TORCH_CHECK(p.ok(), p.error);
  return p;
}

inline torch::Tensor as_bf16(const torch::Tensor& t) {
  return t.to(torch::kBFloat16).contiguous();
}
inline bool aligned16(const torch::Tensor& t) {
  return ((uintptr_t)t.data_ptr() & 15) == 0;
}
// a contiguous bf16 VIEW passes through .contiguous() unchanged, storage
// offset included: an operand at an odd offset of a flat buffer is copied
inline torch::Tensor as_bf16_aligned(const torch::Tensor& t) {
  auto c = as_bf16(t);
  return aligned16(c) ? c : c.clone();
}
inline hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

template <class Fn>
inline void pick_tile(int rows, Fn&& f) {
  if (rows == 16) f(std::integral_constant<int, 16>{});
  else if (rows == 32) f(std::integral_constant<int, 32>{});
  else if (rows == 64) f(std::integral_constant<int, 64>{});
  else TORCH_CHECK(false, "no Conv1D kernel instantiated for rows ", rows);
}
template <class Fn>
inline void pick_act(int act, Fn&& f) {
  switch (act) {
    case ACT_LINEAR: f(std::integral_constant<int, ACT_LINEAR>{}); break;
    case ACT_TANH: f(std::integral_constant<int, ACT_TANH>{}); break;
    case ACT_RELU: f(std::integral_constant<int, ACT_RELU>{}); break;
    case ACT_SIGMOID: f(std::integral_constant<int, ACT_SIGMOID>{}); break;
    default: TORCH_CHECK(false, "unknown activation code ", act);
  }
}

// X [G,B,T,Ck] -> [G,B,T,Cn] through conv1d_tile_kernel<., MODE, ACT>
template <int MODE>
torch::Tensor launch_tile(const ConvPlan& p, const torch::Tensor& xc,
                          const torch::Tensor& Wc, const float* bias, int act,
                          int Ck, int Cn, int k, int d) {
  const int G = xc.size(0), B = xc.size(1), T = xc.size(2);
  TORCH_CHECK(aligned16(xc) && aligned16(Wc),
              "Conv1D operands must be 16-byte aligned");
  TORCH_CHECK((int64_t)B * ceil_div(T, p.rows) < ((int64_t)1 << 31),
              "Conv1D: too many row tiles in one launch");
  TORCH_CHECK(ceil_div((p.rows + (k - 1) * d) * (Ck / 8), 256) <= IMG_IT_MAX,
              "Conv1D image exceeds the per-thread chunk map");
  auto Y = torch::empty({G, B, T, Cn}, xc.options());
  TORCH_CHECK(aligned16(Y), "Conv1D output must be 16-byte aligned");
  g_last_conv = p;
  pick_tile(p.rows, [&](auto R) {
    pick_act(act, [&](auto A) {
      // bwd-data has no epilogue: only its linear instantiation exists
      constexpr int ACT = MODE == 0 ? decltype(A)::value : ACT_LINEAR;
      hipLaunchKernelGGL(
          (conv1d_tile_kernel<decltype(R)::value, MODE, ACT>),
          dim3(p.blocks), dim3(256), p.lds_bytes, cur_stream(),
          (const bf16*)xc.data_ptr(), (const bf16*)Wc.data_ptr(), bias,
          (bf16*)Y.data_ptr(), B, T, Ck, Cn, k, d, p.left,
          p.taps_resident ? 1 : 0, p.chunks, p.per_chunk);
    });
  });
  return Y;
}

// x [G,B,T,Cin]; W [G,k,Cin,Cout]; b [G,Cout] -> y [G,B,T,Cout]
torch::Tensor conv1d_fwd(torch::Tensor x, torch::Tensor W, torch::Tensor b,
                         int64_t act, const std::string& padding,
                         int64_t dilation) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "x must be [G,B,T,Cin] on GPU");
  TORCH_CHECK(W.is_cuda() && W.dim() == 4, "W must be [G,k,Cin,Cout] on GPU");
  auto xc = as_bf16_aligned(x), Wc = as_bf16_aligned(W);
  auto bc = b.to(torch::kFloat32).contiguous();
  const int G = xc.size(0), B = xc.size(1), T = xc.size(2), Cin = xc.size(3);
  const int k = Wc.size(1), Cout = Wc.size(3);
  TORCH_CHECK(Wc.size(0) == G && Wc.size(2) == Cin, "W does not match x");
  TORCH_CHECK(bc.is_cuda() && bc.dim() == 2 && bc.size(0) == G &&
                  bc.size(1) == Cout, "b must be [G,Cout] on GPU");
  const ConvPlan p =
      planned(CONV_FWD, G, B, T, Cin, Cout, k, (int)dilation, padding);
  return launch_tile<0>(p, xc, Wc, bc.data_ptr<float>(), (int)act, Cin, Cout,
                        k, (int)dilation);
}

// dZ [G,B,T,Cout]; W [G,k,Cin,Cout] -> dX [G,B,T,Cin]
torch::Tensor conv1d_bwd_data(torch::Tensor dZ, torch::Tensor W,
                              const std::string& padding, int64_t dilation) {
  TORCH_CHECK(dZ.is_cuda() && dZ.dim() == 4, "dZ must be [G,B,T,Cout] on GPU");
  TORCH_CHECK(W.is_cuda() && W.dim() == 4, "W must be [G,k,Cin,Cout] on GPU");
  auto zc = as_bf16_aligned(dZ), Wc = as_bf16_aligned(W);
  const int G = zc.size(0), B = zc.size(1), T = zc.size(2), Cout = zc.size(3);
  const int k = Wc.size(1), Cin = Wc.size(2);
  TORCH_CHECK(Wc.size(0) == G && Wc.size(3) == Cout, "W does not match dZ");
  const ConvPlan p =
      planned(CONV_BWD_DATA, G, B, T, Cin, Cout, k, (int)dilation, padding);
  return launch_tile<1>(p, zc, Wc, nullptr, ACT_LINEAR, Cout, Cin, k,
                        (int)dilation);
}

// x [G,B,T,Cin]; dZ [G,B,T,Cout] -> {dW [G,k,Cin,Cout], db [G,Cout]} fp32
std::vector<torch::Tensor> conv1d_wgrad(torch::Tensor x, torch::Tensor dZ,
                                        int64_t k64,
                                        const std::string& padding,
                                        int64_t dilation) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "x must be [G,B,T,Cin] on GPU");
  TORCH_CHECK(dZ.is_cuda() && dZ.dim() == 4, "dZ must be [G,B,T,Cout] on GPU");
  auto xc = as_bf16_aligned(x), zc = as_bf16_aligned(dZ);
  const int G = xc.size(0), B = xc.size(1), T = xc.size(2), Cin = xc.size(3);
  const int Cout = zc.size(3), k = (int)k64, d = (int)dilation;
  TORCH_CHECK(zc.size(0) == G && zc.size(1) == B && zc.size(2) == T,
              "dZ does not match x");
  TORCH_CHECK(aligned16(xc) && aligned16(zc),
              "Conv1D operands must be 16-byte aligned");
  const ConvPlan p = planned(CONV_WGRAD, G, B, T, Cin, Cout, k, d, padding);
  auto opts = xc.options().dtype(torch::kFloat32);
  // one chunk writes every element; more add into zeros
  auto dW = p.chunks > 1 ? torch::zeros({G, k, Cin, Cout}, opts)
                         : torch::empty({G, k, Cin, Cout}, opts);
  auto db = p.chunks > 1 ? torch::zeros({G, Cout}, opts)
                         : torch::empty({G, Cout}, opts);
  g_last_conv = p;
  const dim3 grid(G, p.chunks, p.tap_groups);
#define GORDO_CONV_WGRAD_CASE(KF, NF, TG)                                    \
  hipLaunchKernelGGL((conv1d_wgrad_kernel<KF, NF, TG>), grid, dim3(256),     \
                     p.lds_bytes, cur_stream(), (const bf16*)xc.data_ptr(),  \
                     (const bf16*)zc.data_ptr(), dW.data_ptr<float>(),       \
                     db.data_ptr<float>(), B, T, Cin, Cout, k, d, p.left,    \
                     p.per_chunk)
  const int kf2 = wgrad_kf2(Cin), nf2 = wgrad_nf2(Cout);
  if (kf2 == 2 && nf2 == 2) GORDO_CONV_WGRAD_CASE(2, 2, 8);
  else if (kf2 == 2) GORDO_CONV_WGRAD_CASE(2, 4, 4);
  else if (nf2 == 2) GORDO_CONV_WGRAD_CASE(4, 2, 4);
  else GORDO_CONV_WGRAD_CASE(4, 4, 2);
#undef GORDO_CONV_WGRAD_CASE
  return {dW, db};
}

}  // namespace gordo_conv
