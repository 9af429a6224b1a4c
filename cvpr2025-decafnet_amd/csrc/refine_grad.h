// Forward / backward pairs of the refinement stage of PtTransformerEarlyFusionIterative (libs/modeling/model.py:449-455,
// libs/modeling/tcn.py:21-38; refine_grad.hip): the stacking of the first-pass logits fused with refine.conv_1x1, and one
// DilatedResidualLayer on 32 channels.  Token-major (B*T0, 32) fp32 rows like the forward.
//
// Two facts about padded rows of the layer's backward (m[b,t] = 0), both consequences of the reference's own lines:
//   * dz = 0 there (the residual sum is multiplied by the mask, tcn.py:29), but the LayerNorm runs on every row, so dln_b still takes
//     dY of a padded row (and dln_w takes dY * N(0) = 0);
//   * dX is NOT zero there: conv_dilated is a plain nn.Conv1d that does not mask its input (tcn.py:25), so valid neighbours at
//     t -+ dilation read a padded row through their side taps and hand it a gradient.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

constexpr int RG_C = 32;               // channels of the refinement TCN (model.py:424: TCN(L, 32, 32))
constexpr int RG_TILE = 64;            // rows a workgroup handles at a time: a lane owns a row, a wave eight channels
constexpr int RG_SLICE_ROWS = 128;     // rows (of the flat B*T0 index) whose parameter-gradient sums one workgroup forms: a constant, so the
                                       // summation order depends on (B, T0) alone
constexpr int RG_MAX_L = 16;           // pyramid levels of refine_in
constexpr int RG_PITCH = RG_TILE + 1;  // LDS pitch of a channel-major [channel][row] tile: a lane per row and a lane per channel both
                                       // walk the banks without conflict

// one slice's partial sums of the layer: PyTorch layouts, in this order
constexpr int RG_P_WD = 0;                             // (32, 32, 3)
constexpr int RG_P_WP = RG_P_WD + RG_C * RG_C * 3;     // (32, 32)
constexpr int RG_P_BD = RG_P_WP + RG_C * RG_C;
constexpr int RG_P_BP = RG_P_BD + RG_C;
constexpr int RG_P_LNW = RG_P_BP + RG_C;
constexpr int RG_P_LNB = RG_P_LNW + RG_C;
constexpr int RG_P_N = RG_P_LNB + RG_C;                // 4224

struct TcnLayerArgs {
  const float* X;                      // (B*T0, 32)
  const uint8_t* mask;                 // (B*T0) or nullptr
  const float* Wd; const float* bd;    // (32, 32, 3), (32)
  const float* Wp; const float* bp;    // (32, 32), (32)
  const float* lnw; const float* lnb;  // (32), (32)
  float* Y;                            // forward: (B*T0, 32)
  const float* dY;                     // backward: (B*T0, 32)
  float* dX;                           // backward: (B*T0, 32) or nullptr; phase 1 leaves dz there, phase 2 adds the taps
  float* dH;                           // backward scratch (B*T0, 32): the gradient in front of the ReLU, or nullptr (dX not wanted)
  float* part;                         // backward scratch (slices, RG_P_N), or nullptr (no parameter gradient wanted)
  int rows, T0, dil;
  int want_wd, want_wp;                // the two outer products are skipped when their gradient is not wanted
  uint64_t seed; uint32_t site; float p, scale; int b0;
};

struct TcnLayerOuts {
  float* dWd; float* dbd; float* dWp; float* dbp; float* dlnw; float* dlnb;
};

struct RefineInArgs {
  const float* logits1;                // (B, S)
  const uint8_t* mask0;                // (B*T0) or nullptr
  const float* W; const float* b;      // (32, L), (32)
  float* H;                            // forward: (B*T0, 32)
  const float* dH;                     // backward: (B*T0, 32)
  float* dU;                           // backward scratch (B*T0, L): the masked gradient of the stacked input, or nullptr
  float* part;                         // backward scratch (slices, (L + 1) * 32): dW_in as [l][c], then db_in; or nullptr
  int rows, T0, L, S;
  int off[RG_MAX_L + 1];               // level l starts at off[l] of a row of logits1
};

}  // namespace dcf
