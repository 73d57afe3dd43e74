// One nn.LSTM(input_size, H, 1, batch_first=True) layer, uni- or bidirectional, all T padded steps or each row's own length
// (lstm.hip).  Internal header.
#pragma once
#include "common.hpp"

namespace gc {

constexpr int LSTM_H = 128;   // the hidden width the recurrence kernels serve (both reference models hard-code it)

// Every buffer is the caller's, fp32, dense.  nd directions; the weights of the directions are stacked, gate order i, f, g, o:
//   w_ih [nd * 4H][I], w_hh [nd * 4H][H], bias [nd * 4H] (= b_ih + b_hh), h0 / c0 [nd][B][H]
//   out [B][T][nd * H]; gates [B * T][nd * 4H] (the input projection, then -- when csave is given -- the activated gates);
//   csave [B][T][nd * H] = c_t, or nullptr: nothing is kept for a backward (gates is then scratch).
//   lens: device int32 [B] or nullptr (every row has length T).  Packed-sequence semantics: row b is active at t < lens[b]
//   (clamped into [0, T]); an inactive step keeps h and c; out is 0 there (all of out is written); the reverse direction starts
//   at t = lens[b] - 1 from h0 / c0.  gates and csave are NOT written at inactive steps.
//   recurrent: 0 = the recurrent products in fp32; 1 = on bf16 operands, fp32 accumulation (forward h_{t-1} W_hh^T with both
//   factors rounded once to bf16, nearest even; backward dgates_t W_hh likewise; everything stored stays fp32 and unrounded, and
//   the input projection and the gradient products stay the fp32 GEMM layer's).  Any other value is refused.
int lstm_fwd(int B, int T, int I, int nd, const float* x, const float* w_ih, const float* w_hh, const float* bias, const float* h0,
             const float* c0, float* out, float* gates, float* csave, const int* lens, int recurrent, hipStream_t st);
// the recurrent argument of the calling thread's next gcgcn_lstm_fwd / _fwd_len / _bwd / _bwd_len call
// (gcgcn_set_option("lstm_recurrent", v); api.hip): returned and reset to 0
int lstm_recurrent_take();

// Floats of workspace lstm_bwd needs: H_prev [B * T][nd * H], the split-K partials of the weight gradients, the bias gradient's partials.
long lstm_ws_elems(int B, int T, int I, int nd);

// dgates [B * T][nd * 4H] receives the pre-activation gate gradients; dx [B * T][I], dw_ih / dw_hh / db stacked like the weights,
// dh0 / dc0 [nd][B][H] per batch row.  lens as in lstm_fwd (the same values): dgates is 0 at inactive steps (all of it is written), so
// dx is 0 there; dout, gates and csave are not read into any result there, whatever they hold.  recurrent as in lstm_fwd.
int lstm_bwd(int B, int T, int I, int nd, const float* x, const float* w_ih, const float* w_hh, const float* h0, const float* c0,
             const float* out, const float* gates, const float* csave, const float* dout, float* dgates, float* dx, float* dw_ih,
             float* dw_hh, float* db, float* dh0, float* dc0, float* ws, long ws_elems, const int* lens, int recurrent, hipStream_t st);

}  // namespace gc
