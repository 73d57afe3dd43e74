"""Bit-reproducible training steps (GraphModelTail.deterministic / config.deterministic): with the producers' owner-computes
backward (tests/test_producer_det_gpu.py) no kernel of the post-encoder step uses a float atomic, and with the HIP encoder and
front end none of the whole GCGCN_glove step does.  Train mode -- dropout is counter-based, so a seed repeats its masks -- two
steps from the same state: logits, loss and EVERY gradient are equal to the last bit."""
import ctypes

import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, models as M
from lstm_cases import Cfg, doc_tensors, load_model
from test_tail_gpu import _compact_case

pytestmark = pytest.mark.gpu


def _require_symbol():
    """Fails loudly on a library without the deterministic entry (where the flag would be an attribute nobody reads)."""
    out = ctypes.c_int64(-1)
    _lib.call("gcgcn_producer_det_elems", 2, 6, 64, 10, ctypes.cast(ctypes.pointer(out), ctypes.c_void_p))
    assert out.value > 0 and gcgcn_amd.GraphModelTail.deterministic is False


@pytest.mark.parametrize("compact", [False, True], ids=["dense", "compact"])
def test_tail_train_step_repeats_bitwise(gpu_device, compact):
    _require_symbol()
    dev = gpu_device
    ctx, node, table, sen, ph, pt, nv = _compact_case(dev, B=3, N=13, S=3, T=48)          # ragged: n_valid = [13, 9, 12]
    B, N, _ = node.shape
    g = torch.Generator().manual_seed(5)
    ner = (torch.randn(7, 20, generator=g) * 0.3).to(dev)
    ntype = torch.randint(0, 7, (B, N), generator=g).to(dev)
    rel = torch.randint(-10, 11, (B, N, N), generator=g).to(dev)
    labels = (torch.rand(B, N, N, 97, generator=g) < 0.05).float().to(dev)
    torch.manual_seed(3)
    tail = gcgcn_amd.GraphModelTail().to(dev).train()
    tail.deterministic, tail.compact_edges = True, compact
    runs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_() for t in (ctx, node, table, ner)]
        tail.zero_grad(set_to_none=True)
        gcgcn_amd.manual_seed(17)
        logits = tail(leaves[0], leaves[1], None, sen, ph, pt, ntype, rel, leaves[2], leaves[3], n_valid=nv)
        loss = gcgcn_amd.pair_bce_loss(logits, labels, n_valid=nv)
        loss.sum().backward()
        res = {"logits": logits.detach(), "loss": loss.detach()}
        res.update({f"leaf{i}": t.grad for i, t in enumerate(leaves)})
        res.update({n_: p.grad.clone() for n_, p in tail.named_parameters() if p.grad is not None})
        runs.append(res)
    a, b = runs
    assert a.keys() == b.keys() and "producers.0.flat" in a and all(f"leaf{i}" in a for i in range(4))
    assert all(torch.isfinite(v).all() for v in a.values())
    gcgcn_amd.manual_seed(18)                                                          # train mode: another seed, other masks
    with torch.no_grad():
        other = tail(ctx, node, None, sen, ph, pt, ntype, rel, table, ner, n_valid=nv)
    assert not torch.equal(other, a["logits"])
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs (max |diff| {(a[k] - b[k]).abs().max().item():.3e})"


def test_model_train_step_repeats_bitwise(gpu_device):
    """GCGCN_glove at the model_step_c1 sizes, HIP encoder and front end, config.deterministic: every parameter gradient -- the
    softmax-shift biases, whose true gradient is 0 and whose rounding residue used to change sign from run to run, included."""
    _require_symbol()
    dev = gpu_device
    g, sd, _ = load_model(dev)
    cfg = Cfg(g["meta"]["vocab"], "hip")
    cfg.frontend_impl, cfg.deterministic, cfg.keep_prob = "hip", True, 0.8
    docs = [doc_tensors(g["raw"], di, dev) for di in range(g["meta"]["docs"])]
    batch = {k: torch.stack([d[k] for d in docs]) for k in docs[0]}
    labels = torch.stack([torch.from_numpy(g["raw"][f"doc{di}.labels"]) for di in range(len(docs))]).to(dev).float()
    runs = []
    for _ in range(2):
        model = M.GCGCN_glove(cfg).to(dev)
        res = model.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert model.deterministic is True and model.rnn.impl == "hip" and model.frontend_impl == "hip"
        model.train()
        torch.manual_seed(12)
        gcgcn_amd.manual_seed(13)
        loss = gcgcn_amd.pair_bce_loss(model(**batch), labels).sum() / len(docs)
        loss.backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        grads["loss"] = loss.detach()
        runs.append(grads)
    a, b = runs
    assert a.keys() == b.keys() and len(a) > 10 and all(torch.isfinite(v).all() for v in a.values())
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, "gradients that differ between two runs: " + ", ".join(
        f"{k} ({(a[k] - b[k]).abs().max().item():.3e})" for k in bad)
