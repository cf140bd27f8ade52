// Host-only planner of the LSTM scan launches (lstm_seq.hip): which
// kernel family runs for a request, at which row tile, with how much
// LDS and on how many workgroups. Every rule of the dispatch lives
// here and nowhere else: the launchers launch the plan they get, the
// launch record is filled from it, and Python asks it (ops.scan_plan,
// ops.lstm_layer_mode). Plain C++17, no torch / HIP / device call.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>

namespace gordo_lstm {

// cell activation codes (ops/reference.py act_code) and the padded
// K-row length of the h / WhT tiles; lstm_seq.hip asserts both against
// the kernels' own constants
constexpr int ACT_LINEAR = 0, ACT_TANH = 1, ACT_RELU = 2, ACT_SIGMOID = 3;
constexpr int PLAN_LDK = 72;
constexpr size_t LDS_BUDGET = 160 * 1024;

inline const char* act_name(int act) {
  switch (act) {
    case ACT_LINEAR: return "linear";
    case ACT_RELU: return "relu";
    case ACT_SIGMOID: return "sigmoid";
    default: return "tanh";
  }
}

// ---- environment switches, read once per call ----
struct ScanEnv {
  int rows = 0;       // GORDO_LSTM_ROWS when 16, 32 or 64 (A/B), else 0
  bool pipe = true;   // GORDO_LSTM_PIPE: off only for "0"
  bool v1 = false;    // GORDO_LSTM_V1: on only for "1"
  bool v4 = true;     // GORDO_LSTM_V4: off only for "0"

  static ScanEnv read() {
    auto is = [](const char* name, const char* v) {
      const char* e = getenv(name);
      return e && strcmp(e, v) == 0;
    };
    ScanEnv s;
    if (const char* e = getenv("GORDO_LSTM_ROWS")) {
      int r = atoi(e);
      if (r == 16 || r == 32 || r == 64) s.rows = r;
    }
    s.pipe = !is("GORDO_LSTM_PIPE", "0");
    s.v1 = is("GORDO_LSTM_V1", "1");
    s.v4 = !is("GORDO_LSTM_V4", "0");
    return s;
  }
};

// ---- geometry ----
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round32(int n) { return (n + 31) & ~31; }

// pad 4H up to the MFMA K-step (32) plus 8: the K loop's last
// fragment read may touch columns [H4, ru32(H4)); they must exist in
// the row and be zero.
inline int pad_ldg(int h4) { return round32(h4) + 8; }

// smallest row tile whose grid reaches ~2 workgroups per CU: the scans
// are latency-bound chains, so co-resident workgroups on one CU
// overlap each other's stalls (WhT is staged once per launch, so
// smaller tiles do not re-read Wh).
inline int pick_rows(const ScanEnv& env, int G, int B) {
  if (env.rows) return env.rows;
  if (G * ceil_div(B, 64) >= 512) return 64;
  if (G * ceil_div(B, 32) >= 512) return 32;
  return 16;
}

// big-H path: Wh streamed from L2
inline bool big_ok(int H) { return H > 64 && H <= 256 && H % 8 == 0; }
// v4 forward (x-GEMM inside the scan)
inline bool v4_ok(int H, int F) {
  return H <= 64 && H % 8 == 0 && F % 8 == 0 && F <= 128;
}
// v2 (barrier-free, 64-row per-wave blocks) pays only when its grid
// fills the chip: below 256 workgroups the row-tiled kernels win
inline bool v2_fills(int G, int B, int H) {
  return H % 16 == 0 && G * ceil_div(B, 64) >= 256;
}

// ---- dynamic LDS bytes, one function per kernel family ----
// r = row tile, ldg = pad_ldg(4H)
inline size_t lds_fwd_tiled(int r, int H, int ldg) {  // v1, v3
  return (size_t)4 * H * PLAN_LDK * 2 + (size_t)r * PLAN_LDK * 2 +
         (size_t)r * ldg * 2 + (size_t)r * H * 4;
}
inline size_t lds_bwd_tiled(int r, int H, int ldg) {  // v1, v3
  return (size_t)H * ldg * 2 + (size_t)r * ldg * 2 +
         (size_t)r * PLAN_LDK * 2 + (size_t)r * H * 4;
}
inline size_t lds_fwd_v2(int H) {
  return (size_t)4 * H * PLAN_LDK * 2 + (size_t)4 * 16 * PLAN_LDK * 2;
}
inline size_t lds_bwd_v2(int H, int ldg) {
  return (size_t)H * ldg * 2 + (size_t)4 * 16 * ldg * 2;
}
inline size_t lds_big(int r, int H, int ldg) {  // forward and backward
  return (size_t)r * (round32(H) + 8) * 2 + (size_t)r * ldg * 2 +
         (size_t)r * H * 4;
}
// gate_bytes: the pre-activation tile is bf16 for tanh, fp32 otherwise
inline size_t lds_v4(int r, int H, int F, int ldg, int act) {
  const size_t gate_bytes = act == ACT_TANH ? 2 : 4;
  const size_t ldkc = round32(H + F) + 8;
  return (size_t)4 * H * ldkc * 2 + (size_t)r * ldkc * 2 +
         (size_t)r * ldg * gate_bytes + (size_t)ldg * 2 + (size_t)r * H * 4;
}
inline size_t lds_v5(int r, int H, int F, int ldg) {
  return lds_bwd_tiled(r, H, ldg) + (size_t)F * ldg * 2;
}
// F = 0 for the bottom-layer scan (no Wx tile, no dX staging)
inline size_t lds_pipe(int r, int H, int F, int ldg, bool last_only) {
  const size_t ring_row = (size_t)(H / 8) * (last_only ? 6 : 7) * 16;
  return lds_v5(r, H, F, ldg) + 2 * (size_t)r * ring_row + (size_t)r * F * 2;
}

// 64-row tiles halve the per-step Wh L2 re-reads (each workgroup
// streams the whole Wh every timestep): taken whenever the LDS fits
// and the batch fills the tile.
inline int pick_rows_big(int B, int H, int ldg) {
  return B >= 48 && lds_big(64, H, ldg) <= LDS_BUDGET ? 64 : 32;
}

// row tile for the pipelined backward, 0 when it does not apply: the
// switch, the geometry (16-byte rows), 32-bit per-block store offsets
// (T < 2^17), and the LDS budget after halving the tile down to 16
inline int pipe_rows(const ScanEnv& env, int rows, int T, int H, int F,
                     bool has_dx, int ldg, bool last_only) {
  if (!env.pipe) return 0;
  if (H < 8 || H > 64 || H % 8 != 0 || T < 1) return 0;
  if (has_dx && (F < 8 || F > 128 || F % 8 != 0)) return 0;
  if ((size_t)64 * T * 256 >= ((size_t)1 << 31)) return 0;
  while (rows > 16 && lds_pipe(rows, H, F, ldg, last_only) > LDS_BUDGET)
    rows /= 2;
  return lds_pipe(rows, H, F, ldg, last_only) <= LDS_BUDGET ? rows : 0;
}

// ---- request and plan ----
enum ScanEntry {
  FWD = 0,     // ops.lstm_seq_fwd: the public xW route
  FWD_V1,      // forced v2 / v1 (big-H dispatch lives here)
  FWD_V3,      // pipelined forward, directly
  FWD_FUSED,   // v4: x-GEMM inside the scan
  BWD,         // ops.lstm_seq_bwd: the public route
  BWD_V1,      // forced v2 / v1
  BWD_BOTTOM,  // bottom-layer scan: pipe without dX, else v3
  BWD_FUSED,   // dX inside the scan: pipe, else v5
  N_ENTRIES
};
constexpr const char* ENTRY_NAMES[N_ENTRIES] = {
    "fwd", "fwd_v1", "fwd_v3", "fwd_fused",
    "bwd", "bwd_v1", "bwd_bottom", "bwd_fused"};

enum ScanFamily {
  FWD_K1, FWD_K2, FWD_K3, FWD_K4, FWD_BIG,
  BWD_K1, BWD_K2, BWD_K3, BWD_K5, BWD_PIPE, BWD_BIG
};
constexpr const char* FAMILY_NAMES[] = {
    "fwd_v1", "fwd_v2", "fwd_v3", "fwd_v4", "fwd_big",
    "bwd_v1", "bwd_v2", "bwd_v3", "bwd_v5", "bwd_pipe", "bwd_big"};

struct ScanRequest {
  ScanEntry entry;
  int G, B, T, H, F;  // F = 0 on the entries without Wx
  bool last_only;     // backward: dSeq is the last step's dh only
  int act;            // cell activation code
};

// What to launch. rows is the row tile (64 for v2, whose H/16 goes in
// hf); has_dx / last_only are -1 outside the pipelined backward: the
// launch record is these fields as they stand. A refusal carries its
// message in `error` and nothing else.
struct ScanPlan {
  ScanFamily family = FWD_K1;
  int rows = 0, hf = 0, has_dx = -1, last_only = -1, act = ACT_TANH;
  size_t lds_bytes = 0;
  int blocks = 0;
  int ldg = 0;
  std::string error;
  bool ok() const { return error.empty(); }
  const char* family_name() const { return FAMILY_NAMES[family]; }
};

inline ScanPlan refuse(std::string msg) {
  ScanPlan p;
  p.error = std::move(msg);
  return p;
}

inline ScanPlan plan_scan(ScanRequest q, const ScanEnv& env) {
  const int G = q.G, B = q.B, T = q.T, H = q.H;
  const int F = q.entry == FWD_FUSED || q.entry == BWD_FUSED ? q.F : 0;
  const int ldg = pad_ldg(4 * H);
  const bool fwd = q.entry <= FWD_FUSED;
  if (q.act < ACT_LINEAR || q.act > ACT_SIGMOID)
    return refuse("unknown LSTM cell activation code " +
                  std::to_string(q.act));
  // only the v4 forward and the pipelined backward take a cell
  // activation; a tanh kernel is never launched for another one
  auto need_pipe = [&]() {
    return refuse(std::string("cell activation '") + act_name(q.act) +
                  "' needs the pipelined kernel (H % 8 == 0, 8 <= H <= 64, " +
                  (q.entry == BWD_FUSED ? "F % 8 == 0, 8 <= F <= 128, " : "") +
                  "T < 2^17, GORDO_LSTM_PIPE != 0)");
  };
  const bool tanh = q.act == ACT_TANH;

  auto tiled = [&](ScanFamily family, int rows, size_t lds,
                   const char* over) {
    if (lds > LDS_BUDGET) return refuse(over);
    ScanPlan p;
    p.family = family;
    p.rows = rows;
    p.act = q.act;
    p.lds_bytes = lds;
    p.blocks = G * ceil_div(B, rows);
    p.ldg = ldg;
    return p;
  };
  auto pipe = [&](int rows, bool has_dx) {
    ScanPlan p = tiled(BWD_PIPE, rows, lds_pipe(rows, H, F, ldg, q.last_only),
                       "LDS budget exceeded (pipe bwd)");
    p.has_dx = has_dx;
    p.last_only = q.last_only;
    return p;
  };
  auto big = [&]() {
    if (!big_ok(H))
      return refuse(std::string(fwd ? "lstm_seq_fwd_big" : "lstm_seq_bwd_big") +
                    " needs 64 < H <= 256, H % 8 == 0");
    const int rows = pick_rows_big(B, H, ldg);
    return tiled(fwd ? FWD_BIG : BWD_BIG, rows, lds_big(rows, H, ldg),
                 fwd ? "LDS budget exceeded (big fwd)"
                     : "LDS budget exceeded (big bwd)");
  };

  // the public routes choose between the entries below
  if (q.entry == FWD)
    q.entry = env.v1 || H > 64 || v2_fills(G, B, H) ? FWD_V1 : FWD_V3;
  if (q.entry == BWD)
    q.entry = tanh && (env.v1 || H > 64 || v2_fills(G, B, H)) ? BWD_V1
                                                               : BWD_BOTTOM;
  if (!tanh && q.entry != FWD_FUSED && q.entry != BWD_BOTTOM &&
      q.entry != BWD_FUSED)
    return refuse(std::string("entry '") + ENTRY_NAMES[q.entry] +
                  "' takes no cell activation");

  int rows = pick_rows(env, G, B);
  switch (q.entry) {
    case FWD_V1:
    case BWD_V1: {
      if (H > 64) return big();
      if (H % 16 == 0) {  // register-resident gate math, no barriers
        ScanPlan p = tiled(fwd ? FWD_K2 : BWD_K2, 64,
                           fwd ? lds_fwd_v2(H) : lds_bwd_v2(H, ldg),
                           "LDS budget exceeded");
        p.hf = H / 16;
        return p;
      }
      return fwd ? tiled(FWD_K1, rows, lds_fwd_tiled(rows, H, ldg),
                         "LDS budget exceeded")
                 : tiled(BWD_K1, rows, lds_bwd_tiled(rows, H, ldg),
                         "LDS budget exceeded");
    }
    case FWD_V3:
      if (H > 64) return big();  // no v3 there
      return tiled(FWD_K3, rows, lds_fwd_tiled(rows, H, ldg),
                   "LDS budget exceeded");
    case FWD_FUSED:
      if (!v4_ok(H, F)) return refuse("lstm_seq_fwd_fused geometry unsupported");
      while (rows > 16 && lds_v4(rows, H, F, ldg, q.act) > LDS_BUDGET)
        rows /= 2;
      return tiled(FWD_K4, rows, lds_v4(rows, H, F, ldg, q.act),
                   "LDS budget exceeded (v4 fwd)");
    case BWD_BOTTOM:
      if (H > 64) return tanh ? big() : need_pipe();
      if (int prow = pipe_rows(env, rows, T, H, 0, false, ldg, q.last_only))
        return pipe(prow, false);
      if (!tanh) return need_pipe();
      return tiled(BWD_K3, rows, lds_bwd_tiled(rows, H, ldg),
                   "LDS budget exceeded");
    case BWD_FUSED:
      if (H > 64 || F > 128) return refuse("lstm_seq_bwd_fused geometry");
      if (int prow = pipe_rows(env, rows, T, H, F, true, ldg, q.last_only))
        return pipe(prow, true);
      if (!tanh) return need_pipe();
      while (rows > 16 && lds_v5(rows, H, F, ldg) > LDS_BUDGET) rows /= 2;
      return tiled(BWD_K5, rows, lds_v5(rows, H, F, ldg),
                   "LDS budget exceeded (v5 bwd)");
    default:
      return refuse("unknown scan entry");
  }
}

// The engine's question, per layer of a stack: "fused" (x-GEMM inside
// the forward scan, dX inside the backward one), "two_step" (x-GEMM,
// then the xW scan) or "per_step" (per-timestep kernels). One per_step
// layer sends its whole stack per timestep. T plays no part here.
inline const char* layer_mode(const ScanEnv& env, int G, int B, int H, int F,
                              int act) {
  auto ok = [&](ScanEntry entry, int a) {
    return plan_scan({entry, G, B, 1, H, F, false, a}, env).ok();
  };
  const bool fused = env.v4 && ok(FWD_FUSED, act);
  // a non-tanh cell needs both activation-aware kernels
  if (act != ACT_TANH)
    return fused && ok(BWD_FUSED, act) ? "fused" : "per_step";
  if (!ok(FWD, act)) return "per_step";
  // big-H scans pay only once their grid fills the chip: below 256
  // workgroups of 32 rows the per-timestep grouped GEMMs, which split
  // the gate columns over many more workgroups, win
  if (H > 64 && G * ceil_div(B, 32) < 256) return "per_step";
  return fused ? "fused" : "two_step";
}

}  // namespace gordo_lstm
