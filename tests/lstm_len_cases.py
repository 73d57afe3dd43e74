"""What tests/test_lstm_len_cpu.py and tests/test_lstm_len_gpu.py share: the cases with per-row lengths and their float64 reference.

Reference: torch.nn.LSTM on the CPU in float64 over pack_padded_sequence(..., enforce_sorted=False), padded back with
pad_packed_sequence(total_length=T); the inputs are lstm_cases.case's (same weights, initial states and cotangent), the cotangent dy
is applied AS GIVEN, padded positions included (the padded output is a constant 0, so autograd ignores it there); gradients by
autograd.  Computed once per case and shared (lru_cache); nobody writes to it.  The bound is lstm_cases' (the project's own)."""
import functools

import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from lstm_cases import H, case, frac_of_bound, param_names, worst  # noqa: F401  (re-exported for the two test files)

# (B, T, I, lens, nd).  The 16-row tile's bound Lt is the largest length among its rows:
CASES = [
    (1, 1, 1, (1,), 2),                                                   # the smallest call
    (3, 5, 7, (5, 1, 3), 2),                                              # a full row, a one-step row, one in between
    (17, 3, 140, tuple([2, 1] * 8) + (3,), 2),                            # first tile Lt = 2 < T, second tile runs T
    (17, 3, 140, tuple([3, 2, 1, 3] * 4) + (1,), 2),                      # the other way round: the second tile's Lt = 1 < T
    (16, 4, 140, (4,) * 16, 2),                                           # all lengths T: nothing is padded
    (33, 37, 140, tuple((7 * i) % 37 + 1 for i in range(33)), 2),         # three tiles, every row its own length
    (33, 6, 140, tuple([5, 3, 1, 4] * 4) + tuple([4, 2, 1, 3] * 4) + (6,), 2),   # tiles with Lt = 5 (odd), 4 (even), 6: both parities
                                                                                 # of the double buffers at the loop's last step
    (2, 512, 140, (512, 200), 2),                                         # the model's length
    (17, 5, 140, tuple((3 * i) % 5 + 1 for i in range(17)), 1),           # unidirectional
]
IDS = [f"{B}x{T}x{I}-nd{nd}-{'full' if min(lens) == T else 'min%d' % min(lens)}-{k}" for k, (B, T, I, lens, nd) in enumerate(CASES)]


def run_torch_packed(c, nd, lens, dtype, device="cpu"):
    """nn.LSTM over the packed sequence, forward + backward in `dtype`: {"out", "dx", "dh0", "dc0", "d<param>"...}."""
    B, T, I = c["x"].shape
    rnn = nn.LSTM(I, H, 1, bidirectional=nd == 2, batch_first=True).to(device=device, dtype=dtype)
    with torch.no_grad():
        for n in param_names(nd):
            getattr(rnn, n).copy_(c[n])
    # clones: the case's tensors are shared (lru_cache), and .to() of a float32 CPU tensor is the tensor itself
    x, h0, c0 = (c[k].detach().to(device=device, dtype=dtype).clone().requires_grad_() for k in ("x", "h0", "c0"))
    packed = pack_padded_sequence(x, torch.tensor(lens, dtype=torch.int64), batch_first=True, enforce_sorted=False)
    out, _ = rnn(packed, (h0.expand(-1, B, -1).contiguous(), c0.expand(-1, B, -1).contiguous()))
    out, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    out.backward(c["dy"].to(device=device, dtype=dtype))
    res = {"out": out.detach(), "dx": x.grad, "dh0": h0.grad, "dc0": c0.grad}
    res.update({"d" + n: getattr(rnn, n).grad for n in param_names(nd)})
    return res


@functools.lru_cache(maxsize=None)
def reference(B, T, I, lens, nd=2, seed=0):
    return run_torch_packed(case(B, T, I, nd, seed), nd, lens, torch.float64)


def padding_mask(B, T, lens):
    """bool [B, T]: True at the padded positions."""
    return torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
