// The level-0 embedding stage of the video backbone as ONE kernel (video_net.py:133-151): embd_fc, [MaskedConv1D(k3) -> LayerNorm ->
// ReLU] x 2 and + pe * mask over the rows of pyramid level 0, at E = 256 in the f16x3 mode.  The kernel is the head chain's body
// (head_chain.hip) with other ends.  embd_fc has no nonlinearity behind it, so it is folded into the first convolution once per
// parameter set (engine_model.hip, fold_embd):
//   y[r] = sum_t m[r + t] u_t (W'_t x[r + t] + c_t),   W'_t = Wc_t Wfc diag(g),   c_t = Wc_t (Wfc b + b_fc)
// with m the row validity, u_t the sequence-edge test (both in the neighbour flags) and (g, b) the affine of fusion.ln_out where the
// kernel normalises the rows itself (ln_in), 1 and 0 where the rows come normalised.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

struct EmbdChainArgs {
  const float* X;               // [rows][ldx] level-0 rows: the raw stream (ln_in = 1) or fusion.ln_out's output (ln_in = 0)
  int64_t ldx;
  const uint8_t* nbr;           // [rows] bit0 row usable, bit1 left neighbour usable, bit2 right (k_pyramid_masks / launch_rowflags)
  const unsigned short* W1c;    // chain image of the folded first convolution W' (launch_split_chain3)
  const unsigned short* W2c;    // ... of embd_convs[1]
  const float* cb;              // [3][C] the folded bias c_t
  const float* ln1_w; const float* ln1_b; const float* ln2_w; const float* ln2_b;   // embd_norms, [C]
  const float* pe;              // [>= T][C] position encoding, or nullptr
  float* Y;                     // [rows][ldy]; never X: neighbouring windows read each other's halo rows
  int64_t ldy;
  int rows, T;                  // T: rows per sequence (pe index = row % T)
  int ln_in;                    // 1: LayerNorm without affine (eps 1e-5) on the loaded rows
  unsigned* status;             // sticky numerics word (GemmArgs::status)
};

bool embd_chain_supports(int C);                     // C = 256
int launch_embd_chain(const EmbdChainArgs& a, hipStream_t stream);

}  // namespace dcf
