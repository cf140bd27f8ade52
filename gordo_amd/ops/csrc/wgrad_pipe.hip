// Whole-tile grouped weight-grad for MI355X (gfx950, CDNA4):
//   dW[g, K, N] (fp32) = A[g, M, K]^T @ dZ[g, M, N],  db[g, N] = colsum(dZ)
// for K <= 128, N <= 256. The dispatch and the fallback kernel
// (grouped_wgrad_kernel, 64x64 tiles) live in gordo_kernels.hip.
//
// Design (docs/kernels.md, "Whole-tile weight-grad"):
//  * One 256-thread workgroup owns the WHOLE [K, N] output of one model
//    for one M-chunk, so every operand byte is requested once per launch.
//    4 waves in a 2x2 layout; a wave owns KF2 x NF2 fragments of 16x16.
//  * Every global read is a row-contiguous 16-byte chunk. The tile goes
//    into LDS row-major ([m][k] and [m][n]) with ds_write_b128, exactly
//    as it arrives; the transposition both MFMA operands need (they are
//    column reads of the row-major images) happens in ds_read_b64_tr_b16.
//  * The A operand may come from two sources: columns [0, K1) from A1
//    (rows as-is) and [K1, K) from A2 read at row gm-1, zero where
//    gm % T == 0 (the h_{t-1} addressing of the recurrent weight-grad).
//  * 32-row m-step, double-buffered images, ONE barrier per step: the
//    next step's global loads are issued before the MFMA phase and
//    written to the other buffer after it.
//  * db comes from the same LDS image: one extra MFMA per n-fragment
//    with an all-ones A operand (no second pass over dZ, no VALU
//    unpacking), split between the two k-waves.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>

namespace gordo_wgrad {

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int MSTEP = 32;     // rows of M per step (one MFMA k-depth)
constexpr int MS = MSTEP;
constexpr int ROW_PAD = 32;   // bytes of padding per image row

// ---- LDS image addressing (host/device, checked at compile time) ----
// Row stride of a [MS][cols] bf16 image. cols is a multiple of 32, so
// cols*2 is a multiple of 64 B and the stride is an ODD multiple of
// 32 B: 8 consecutive rows start 8 banks apart, all distinct mod 64.
constexpr __host__ __device__ int img_stride(int cols) {
  return cols * 2 + ROW_PAD;
}
// byte offset of 16-byte chunk `ch` of row `row` (the ds_write_b128)
constexpr __host__ __device__ int img_store_off(int stride, int row, int ch) {
  return row * stride + ch * 16;
}
// byte address lane `lane` supplies to transposed read `rd` (0/1) of
// the 16 columns of fragment `frag`. Group g = lane/16 reads rows
// 16*rd + 4g .. +3, so a 32-lane half covers 8 CONSECUTIVE rows; lane
// 4q+p of the group supplies row q, columns 4p..4p+3, and lane i
// receives column i with row q in element q. Element e = 4*rd + q of
// lane (g, i) is therefore image[16*rd + 4g + q][16*frag + i] for the A
// and the dZ image alike, which is all the MFMA needs of the m order.
constexpr __host__ __device__ int img_tr_off(int stride, int lane, int frag,
                                             int rd) {
  const int g = (lane >> 4) & 3, q = (lane >> 2) & 3, p = lane & 3;
  return (16 * rd + 4 * g + q) * stride + (frag * 16 + 4 * p) * 2;
}
// every transposed read of an image of `cols` columns: 8-byte aligned,
// inside the image, and no two lanes of a 32-lane half on one bank
// (bank = (addr/4) % 64, two banks per 8-byte lane access)
constexpr bool img_tr_reads_ok(int cols) {
  const int stride = img_stride(cols);
  for (int frag = 0; frag < cols / 16; ++frag)
    for (int rd = 0; rd < 2; ++rd)
      for (int half = 0; half < 2; ++half) {
        int used[64] = {};
        for (int l = 0; l < 32; ++l) {
          const int off = img_tr_off(stride, half * 32 + l, frag, rd);
          if (off % 8 != 0 || off < 0 || off + 8 > MS * stride) return false;
          for (int d = 0; d < 2; ++d)
            if (used[(off / 4 + d) % 64]++) return false;
        }
      }
  return true;
}
static_assert(img_tr_reads_ok(64) && img_tr_reads_ok(128) &&
                  img_tr_reads_ok(192) && img_tr_reads_ok(256),
              "transposed reads must be aligned, in bounds, conflict-free");

// one MFMA operand: the two transposed reads of a fragment's 32 rows
__device__ __forceinline__ bf16x8 tr_operand(const char* img, int off,
                                             int stride) {
  typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
  i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)(img + off));
  i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_i16x4*)(img + off + 16 * stride));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// KF2 / NF2: 16x16 fragments per wave along K / N (the workgroup holds
// 2*KF2 x 2*NF2). Padding fragments multiply zero-filled LDS.
template <int KF2, int NF2>
__global__ __launch_bounds__(256) void grouped_wgrad_pipe_kernel(
    const bf16* __restrict__ A1, const bf16* __restrict__ A2,
    const bf16* __restrict__ dZ, float* __restrict__ dW,
    float* __restrict__ db, int M, int N, int K, int K1, int T, int mchunk) {
  constexpr int KC = KF2 * 32, NC = NF2 * 32;      // image columns
  constexpr int SA = img_stride(KC), SZ = img_stride(NC);
  constexpr int A_BYTES = MS * SA, BUF = A_BYTES + MS * SZ;
  constexpr int A_CH = KC / 8, Z_CH = NC / 8;      // 16-byte chunks per row
  constexpr int A_IT = MS * A_CH / 256, Z_IT = MS * Z_CH / 256;
  static_assert(MS * A_CH % 256 == 0 && MS * Z_CH % 256 == 0, "chunk map");
  static_assert(2 * BUF <= 64 * 1024, "static LDS");
  __shared__ __attribute__((aligned(16))) char sm[2 * BUF];

  const int g = blockIdx.x;
  const int m_begin = blockIdx.y * mchunk;
  const int m_end = (m_begin + mchunk < M) ? m_begin + mchunk : M;
  const int K2 = K - K1;
  const bf16* Zg = dZ + (size_t)g * M * N;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // wave-uniform by construction; readfirstlane lets the compiler keep
  // the per-wave choices below in scalar registers and scalar branches
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wid & 1, wn = wid >> 1;

  // ---- per-thread chunk descriptors (constant over the m loop) ----
  // mode 0: padding chunk (always zero), 1: A1 row gm, 2: A2 row gm-1
  const bf16* a_src[A_IT];
  int a_ld[A_IT], a_mode[A_IT], a_row[A_IT], a_off[A_IT];
  int a_t[A_IT];  // (row of the NEXT stage_load) % T, kept incrementally
  const int t_step = MS % T;
#pragma unroll
  for (int i = 0; i < A_IT; ++i) {
    const int idx = tid + 256 * i;
    const int row = idx / A_CH, c = (idx % A_CH) * 8;
    a_row[i] = row;
    a_t[i] = (m_begin + row) % T;
    a_off[i] = img_store_off(SA, row, idx % A_CH);
    if (c < K1) {
      a_mode[i] = 1; a_ld[i] = K1;
      a_src[i] = A1 + (size_t)g * M * K1 + c;
    } else if (c < K) {
      a_mode[i] = 2; a_ld[i] = K2;
      a_src[i] = A2 + (size_t)g * M * K2 + (c - K1);
    } else {
      a_mode[i] = 0; a_ld[i] = 0;
      a_src[i] = Zg;  // any valid 16-byte aligned address
    }
  }
  const bf16* z_src[Z_IT];
  int z_row[Z_IT], z_off[Z_IT];
  bool z_col_ok[Z_IT];
#pragma unroll
  for (int i = 0; i < Z_IT; ++i) {
    const int idx = tid + 256 * i;
    const int row = idx / Z_CH, c = (idx % Z_CH) * 8;
    z_row[i] = row;
    z_off[i] = A_BYTES + img_store_off(SZ, row, idx % Z_CH);
    z_col_ok[i] = c < N;
    z_src[i] = Zg + (c < N ? c : 0);
  }

  u32x4 a_reg[A_IT], z_reg[Z_IT];
  bool a_ok[A_IT], z_ok[Z_IT];

  // STAGE_LOAD: clamped addresses, never a branch around a load; the
  // zero-select happens at the LDS write.
  // Called for m_begin, m_begin + MS, ... in order (a_t relies on it).
  auto stage_load = [&](int m0) {
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
      const int gm = m0 + a_row[i];
      const bool shifted = a_mode[i] == 2;
      int r = gm < M ? gm : M - 1;
      r = (shifted && r > 0) ? r - 1 : r;
      // t == 0 -> h_prev is zero
      a_ok[i] = gm < m_end && a_mode[i] != 0 && !(shifted && a_t[i] == 0);
      const int t_next = a_t[i] + t_step;
      a_t[i] = t_next >= T ? t_next - T : t_next;
      a_reg[i] = *reinterpret_cast<const u32x4*>(a_src[i] +
                                                 (size_t)r * a_ld[i]);
    }
#pragma unroll
    for (int i = 0; i < Z_IT; ++i) {
      const int gm = m0 + z_row[i];
      const int r = gm < M ? gm : M - 1;
      z_ok[i] = gm < m_end && z_col_ok[i];
      z_reg[i] = *reinterpret_cast<const u32x4*>(z_src[i] + (size_t)r * N);
    }
  };
  auto stage_write = [&](char* buf) {
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < A_IT; ++i)
      *reinterpret_cast<u32x4*>(buf + a_off[i]) = a_ok[i] ? a_reg[i] : zero;
#pragma unroll
    for (int i = 0; i < Z_IT; ++i)
      *reinterpret_cast<u32x4*>(buf + z_off[i]) = z_ok[i] ? z_reg[i] : zero;
  };

  f32x4 acc[KF2][NF2] = {};
  f32x4 acc_db[NF2 / 2] = {};
  const short one_bf16 = 0x3F80;
  const bf16x8 ones = {one_bf16, one_bf16, one_bf16, one_bf16,
                       one_bf16, one_bf16, one_bf16, one_bf16};

  // transposed-read offsets of this lane's first fragments
  const int a_tr0 = img_tr_off(SA, lane, wk * KF2, 0);
  const int z_tr0 = A_BYTES + img_tr_off(SZ, lane, wn * NF2, 0);

  stage_load(m_begin);
  stage_write(sm);
  __syncthreads();

  int cur = 0;
  for (int m0 = m_begin; m0 < m_end; m0 += MS) {
    const char* rbuf = sm + cur * BUF;
    // the last trip loads clamped rows it then writes as zeros: the
    // loop body stays branch-free
    stage_load(m0 + MS);
    __builtin_amdgcn_sched_barrier(0);

    bf16x8 a[KF2];
#pragma unroll
    for (int i = 0; i < KF2; ++i) {
      a[i] = tr_operand(rbuf, a_tr0 + i * 32, SA);
    }
#pragma unroll
    for (int j = 0; j < NF2; ++j) {
      const bf16x8 b = tr_operand(rbuf, z_tr0 + j * 32, SZ);
#pragma unroll
      for (int i = 0; i < KF2; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b,
                                                            acc[i][j], 0, 0, 0);
      // bias-grad: wave wk sums its half of the wave's n-fragments
      // (wave-uniform branch; the LDS reads above are outside it)
      if ((j >= NF2 / 2) == (wk == 1))
        acc_db[j % (NF2 / 2)] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            ones, b, acc_db[j % (NF2 / 2)], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    stage_write(sm + (cur ^ 1) * BUF);
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue ----
  float* Wg = dW + (size_t)g * K * N;
  const bool single_chunk = gridDim.y == 1;
  const int l15 = lane & 15, rq = (lane >> 4) * 4;
#pragma unroll
  for (int j = 0; j < NF2; ++j) {
    const int col = (wn * NF2 + j) * 16 + l15;
    if (col >= N) continue;
    if ((j >= NF2 / 2) == (wk == 1) && rq == 0) {
      // all 16 rows of the ones-product hold the column sum; row 0
      atomicAdd(&db[(size_t)g * N + col], acc_db[j % (NF2 / 2)][0]);
    }
#pragma unroll
    for (int i = 0; i < KF2; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = (wk * KF2 + i) * 16 + rq + r;
        if (row >= K) continue;
        if (single_chunk)
          Wg[(size_t)row * N + col] = acc[i][j][r];
        else
          atomicAdd(&Wg[(size_t)row * N + col], acc[i][j][r]);
      }
    }
  }
}

// ---- host side ----
bool pipe_shape_ok(int K, int K1, int N) {
  return K >= 8 && K <= 128 && N >= 8 && N <= 256 && K1 % 8 == 0 &&
         (K - K1) % 8 == 0 && N % 8 == 0;
}

template <int KF2, int NF2>
static void launch_one(const bf16* A1, const bf16* A2, const bf16* dZ,
                       float* dW, float* db, int G, int M, int N, int K,
                       int K1, int T, int mchunk, int nchunks,
                       hipStream_t stream) {
  hipLaunchKernelGGL((grouped_wgrad_pipe_kernel<KF2, NF2>), dim3(G, nchunks),
                     dim3(256), 0, stream, A1, A2, dZ, dW, db, M, N, K, K1,
                     T > 0 ? T : 1, mchunk);
}

// A1: [G, M, K1] (rows as-is; may be null when K1 == 0), A2: [G, M,
// K-K1] read at row-1 with (row % T == 0) zero (null when K1 == K).
// The caller has checked pipe_shape_ok and 16-byte operand alignment.
void launch_pipe(const void* A1, const void* A2, const void* dZ, float* dW,
                 float* db, int G, int M, int N, int K, int K1, int T,
                 int mchunk, int nchunks, hipStream_t stream) {
  const bf16* a1 = (const bf16*)A1;
  const bf16* a2 = (const bf16*)A2;
  const bf16* z = (const bf16*)dZ;
  const int nf2 = (N + 63) / 64 * 2;  // 2, 4, 6, 8
#define GORDO_WGRAD_CASE(KF, NF)                                           \
  launch_one<KF, NF>(a1, a2, z, dW, db, G, M, N, K, K1, T, mchunk,        \
                     nchunks, stream)
  if (K <= 64) {
    switch (nf2) {
      case 2: GORDO_WGRAD_CASE(2, 2); break;
      case 4: GORDO_WGRAD_CASE(2, 4); break;
      case 6: GORDO_WGRAD_CASE(2, 6); break;
      default: GORDO_WGRAD_CASE(2, 8); break;
    }
  } else {
    switch (nf2) {
      case 2: GORDO_WGRAD_CASE(4, 2); break;
      case 4: GORDO_WGRAD_CASE(4, 4); break;
      case 6: GORDO_WGRAD_CASE(4, 6); break;
      default: GORDO_WGRAD_CASE(4, 8); break;
    }
  }
#undef GORDO_WGRAD_CASE
}

}  // namespace gordo_wgrad
