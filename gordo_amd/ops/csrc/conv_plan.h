// Host-only planner of the grouped Conv1D launches (conv1d.hip): which
// kernel runs for a request, at which row tile, with the taps resident
// in LDS or on the two-tap ring, with how much LDS and on how many
// workgroups. Every rule of the dispatch lives here: the launchers
// launch the plan they get, the launch record is the plan, and Python
// asks it (ops.conv1d_plan, ops.conv1d_refusal). Plain C++17, no torch /
// HIP / device call.
#pragma once

#include <cstddef>
#include <string>

namespace gordo_conv {

constexpr size_t LDS_BUDGET = 160 * 1024;
// grid target of all three kernels: about two workgroups per CU, the
// figure grouped_wgrad_pipe_kernel aims for
constexpr int TARGET_WGS = 512;
// a weight-grad chunk shorter than this costs more in atomics and
// zero-fill than it gains (the whole-tile weight-grad's measurement)
constexpr int WGRAD_MIN_CHUNK_ROWS = 512;
constexpr int WGRAD_ROWS = 32;       // rows per step: one MFMA k-depth
constexpr int WGRAD_ACC_FRAGS = 32;  // 16x16 fp32 fragments per wave
constexpr int MAX_HALO = 64, MAX_TAPS = 8, MAX_CH = 128;

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round16(int n) { return (n + 15) & ~15; }
inline int round32(int n) { return (n + 31) & ~31; }

enum ConvEntry { CONV_FWD = 0, CONV_BWD_DATA, CONV_WGRAD, N_CONV_ENTRIES };
constexpr const char* CONV_ENTRY_NAMES[N_CONV_ENTRIES] = {"fwd", "bwd_data",
                                                          "wgrad"};
constexpr const char* CONV_FAMILY_NAMES[N_CONV_ENTRIES] = {
    "conv1d_fwd", "conv1d_bwd_data", "conv1d_wgrad"};

inline int entry_code(const std::string& name) {
  for (int e = 0; e < N_CONV_ENTRIES; ++e)
    if (name == CONV_ENTRY_NAMES[e]) return e;
  return -1;
}

// ---- geometry ----
// zero rows in front of a window: Keras "causal" puts the whole halo
// there, TensorFlow's "same" the smaller half (the remainder goes right)
inline int left_pad(bool causal, int k, int d) {
  return causal ? (k - 1) * d : ((k - 1) * d) / 2;
}

// the row tile that wastes the fewest padded rows for T, ties to the
// larger: T = 144 -> 16, T = 64 -> 64
inline int pick_rows(int T) {
  int best = 16, waste = ceil_div(T, 16) * 16 - T;
  for (int r : {32, 64}) {
    const int w = ceil_div(T, r) * r - T;
    if (w <= waste) best = r, waste = w;
  }
  return best;
}

// LDS row length (bf16) of an image or weight-panel row over `c`
// contracted channels: padded to the MFMA k-step, plus 8 (the stride is
// then 4 * odd dwords; docs/kernels.md, "Grouped Conv1D")
inline int tile_ldk(int c) { return round32(c) + 8; }

// forward / bwd-data: ck contracted channels, cn output channels.
// weight panels [slots][round16(cn)][ldk] | image [2][rows + halo][ldk] |
// output staging [2][rows][cn + 8], all bf16
inline size_t lds_tile(int rows, int ck, int cn, int k, int halo,
                       bool resident) {
  const size_t ldk = tile_ldk(ck);
  return (size_t)(resident ? k : 2) * round16(cn) * ldk * 2 +
         (size_t)2 * (rows + halo) * ldk * 2 +
         (size_t)2 * rows * (cn + 8) * 2;
}

// weight-grad: fragments per wave along Cin / Cout (2 x 2 waves), and
// how many taps' accumulators one workgroup holds
inline int wgrad_kf2(int cin) { return cin <= 64 ? 2 : 4; }
inline int wgrad_nf2(int cout) { return cout <= 64 ? 2 : 4; }
inline int wgrad_tap_group(int cin, int cout) {
  return WGRAD_ACC_FRAGS / (wgrad_kf2(cin) * wgrad_nf2(cout));
}
// X image [2][32 + halo of one tap group][KC * 2 + 32 B] | dZ image
// [2][32][NC * 2 + 32 B]
inline size_t lds_wgrad(int cin, int cout, int taps, int d) {
  const size_t sa = wgrad_kf2(cin) * 64 + 32, sz = wgrad_nf2(cout) * 64 + 32;
  return 2 * ((size_t)(WGRAD_ROWS + (taps - 1) * d) * sa + WGRAD_ROWS * sz);
}

// What to launch. A refusal carries its message in `error` and nothing
// else. taps_resident: forward / bwd-data keep all k weight panels in
// LDS (else the two-tap ring); weight-grad holds all k taps'
// accumulators in one workgroup (else tap groups on gridDim.z).
struct ConvPlan {
  ConvEntry entry = CONV_FWD;
  int rows = 0;
  bool taps_resident = true;
  size_t lds_bytes = 0;
  int blocks = 0, chunks = 0;
  // geometry for the launcher
  int left = 0;       // zero rows in front (bwd-data: mirrored)
  int per_chunk = 0;  // items (fwd / bwd-data) or windows (wgrad) per chunk
  int tap_group = 0, tap_groups = 0;  // wgrad
  std::string error;
  bool ok() const { return error.empty(); }
  const char* family_name() const { return CONV_FAMILY_NAMES[entry]; }
};

inline ConvPlan refuse_conv(std::string msg) {
  ConvPlan p;
  p.error = std::move(msg);
  return p;
}

inline ConvPlan plan_conv1d(int entry, int G, int B, int T, int Cin, int Cout,
                            int k, int d, const std::string& padding) {
  auto bad_ch = [](int c) { return c < 8 || c > MAX_CH || c % 8 != 0; };
  if (entry < 0 || entry >= N_CONV_ENTRIES)
    return refuse_conv("unknown Conv1D entry (fwd, bwd_data, wgrad)");
  if (padding != "same" && padding != "causal")
    return refuse_conv("Conv1D padding must be 'same' or 'causal', got '" +
                       padding + "'");
  if (bad_ch(Cin) || bad_ch(Cout))
    return refuse_conv(
        "Conv1D needs 8 <= channels <= 128 in multiples of 8, got Cin = " +
        std::to_string(Cin) + ", Cout = " + std::to_string(Cout));
  if (k < 1 || k > MAX_TAPS)
    return refuse_conv("Conv1D needs 1 <= kernel_size <= 8, got " +
                       std::to_string(k));
  if (d < 1 || (k - 1) * d > MAX_HALO)
    return refuse_conv(
        "Conv1D needs dilation >= 1 and (kernel_size - 1) * dilation <= 64, "
        "got kernel_size = " + std::to_string(k) + ", dilation = " +
        std::to_string(d));
  if (T < 1 || T >= (1 << 17))
    return refuse_conv("Conv1D needs 1 <= T < 2^17, got T = " +
                       std::to_string(T));
  if (G < 1 || B < 1) return refuse_conv("Conv1D needs G, B >= 1");

  const int halo = (k - 1) * d;
  const int left = left_pad(padding == "causal", k, d);
  ConvPlan p;
  p.entry = (ConvEntry)entry;

  if (entry == CONV_WGRAD) {
    const int tg = wgrad_tap_group(Cin, Cout);
    p.rows = WGRAD_ROWS;
    p.tap_group = tg < k ? tg : k;
    p.tap_groups = ceil_div(k, tg);
    p.taps_resident = p.tap_groups == 1;
    p.left = left;
    p.lds_bytes = lds_wgrad(Cin, Cout, p.tap_group, d);
    if (p.lds_bytes > LDS_BUDGET)
      return refuse_conv("LDS budget exceeded (conv1d wgrad)");
    // whole windows per chunk, no chunk under WGRAD_MIN_CHUNK_ROWS rows
    const int target = TARGET_WGS / (G * p.tap_groups);
    int wpc = ceil_div(B, target > 1 ? target : 1);
    const int min_w = ceil_div(WGRAD_MIN_CHUNK_ROWS, T);
    if (wpc < min_w) wpc = min_w;
    if (wpc > B) wpc = B;
    p.per_chunk = wpc;
    p.chunks = ceil_div(B, wpc);
    p.blocks = G * p.chunks * p.tap_groups;
    return p;
  }

  // forward contracts Cin into Cout, bwd-data Cout into Cin
  const int ck = entry == CONV_FWD ? Cin : Cout;
  const int cn = entry == CONV_FWD ? Cout : Cin;
  const int rows0 = pick_rows(T);
  // all taps beside the image, halving the tile while over budget; else
  // the two-tap ring, by the same halving rule
  bool resident = true;
  int rows = rows0;
  while (rows > 16 && lds_tile(rows, ck, cn, k, halo, true) > LDS_BUDGET)
    rows /= 2;
  if (lds_tile(rows, ck, cn, k, halo, true) > LDS_BUDGET) {
    resident = false;
    rows = rows0;
    while (rows > 16 && lds_tile(rows, ck, cn, k, halo, false) > LDS_BUDGET)
      rows /= 2;
    if (lds_tile(rows, ck, cn, k, halo, false) > LDS_BUDGET)
      return refuse_conv("LDS budget exceeded (conv1d, 16-row tile)");
  }
  p.rows = rows;
  p.taps_resident = resident;
  p.lds_bytes = lds_tile(rows, ck, cn, k, halo, resident);
  p.left = entry == CONV_FWD ? left : halo - left;
  // a workgroup owns one model and a contiguous range of (b, tile) items
  const long items = (long)B * ceil_div(T, rows);
  const int target = TARGET_WGS / G > 1 ? TARGET_WGS / G : 1;
  const long ipc = (items + target - 1) / target;
  p.per_chunk = (int)ipc;
  p.chunks = (int)((items + ipc - 1) / ipc);
  p.blocks = G * p.chunks;
  return p;
}

}  // namespace gordo_conv
