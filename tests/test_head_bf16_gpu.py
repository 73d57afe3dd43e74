"""``classifier_head(..., matmul="bf16")`` on the device: the bilinear passes of csrc/head_bf16.hip (v_mfma_f32_32x32x16_bf16) against
the float64 run of the definition ``gcgcn_amd.functional.Bf16HeadBilinearFn``, through the C ABI (gcgcn_head_fwd / gcgcn_head_bwd announced
with head_matmul = 1, every buffer NaN-filled) and through the Python layers.  Bounds, references and the harness: tests/head_bf16_cases.py.

Measured on an MI355X (worst fraction of the bound over all cases of a test; no bound raised):
  per pass, derived bound  : logits 0.00005, d eh 0.0040, d et 0.0043 (both at R = 1), d bili_layer_01.weight 0.15,
                             d classification_layer_01.weight 0.11; the fp32 head breaks the two weight-gradient bounds on 0.87-1.00
                             of their elements and, at R = 1, the d eh / d et bounds on 0.96
  end to end, c = 5e-3     : logits 0.017, d feats 0.011, d dense_layer 0.007, d bili_layer_01.weight 0.16,
                             d classification_layer_01.weight 0.087, d ner_emb 0.009, d dis_embed 0.010; model logits 0.32
"""
import ctypes

import pytest
import torch

import head_bf16_cases as C
from gcgcn_amd import _lib

pytestmark = pytest.mark.gpu

# (B, N, R, nf, n_valid): 2 live pairs in one guarded tile; 50 rows; 81 rows (past 64); 288 rows (past 128, two K splits of the weight
# gradient, a partial tile); R at 97 (a fourth block with one column), 96 (three blocks), 33 (two), 1; compacted rows of a ragged batch
PASS_CASES = [(1, 2, 97, 1, None), (2, 5, 33, 3, None), (1, 9, 96, 3, None), (2, 12, 97, 3, None), (1, 9, 1, 1, None), (2, 5, 97, 1, None),
              (3, 12, 97, 3, (12, 7, 0))]
RAGGED = [(3, 12, (12, 7, 0)), (3, 12, (1, 1, 1)), (2, 16, (16, 3))]


def _id(case):
    B, N, R, nf, nv = case
    return f"B={B} N={N} R={R} nf={nf}" + ("" if nv is None else f" nv={list(nv)}")


def _live_rows(c, t):
    """[B,N,N,.] -> the pair rows the passes work on: every slot, or the live pairs in (b, i, j) order."""
    return t[c.pair] if c.ragged else t.reshape(c.B * c.N * c.N, -1)


@pytest.mark.parametrize("case", PASS_CASES, ids=_id)
def test_each_pass_meets_the_derived_bound_and_the_fp32_head_does_not(gpu_device, case):
    """Forward, d eh, d et, d W_b and d W_c of the bf16 head against float64 over the operands the device rounded, each element under
    2^-23 (K + 2) sum |A^||B^|; the fp32 head (not announced, same buffers) breaks that bound on most elements of the two weight
    gradients, and at R = 1 (K = 129) of d eh and d et too.  This is the test that fails when an fp32 kernel stands behind the switch."""
    B, N, R, nf, nv = case
    c = C.make_case(B, N, R, nv=nv, nf=nf)
    dout = _live_rows(c, c.cot)
    res = {}
    for matmul in (1, 0):
        got, ws = C.run_abi(c, gpu_device, matmul)
        if matmul == 1:
            assert all(torch.isfinite(v).all() for v in ws.values()), "a workspace row of a live pair is not finite"
            ref, mag = C.pass_reference(ws["eh"], ws["et"], c.sd, dout)
            factor = {"d eh": 1 - ws["eh"].double() ** 2, "d et": 1 - ws["et"].double() ** 2}
        obs = {"logits": _live_rows(c, got["logits"].cpu()), "d eh": ws["g eh"], "d et": ws["g et"]}
        obs.update({"d " + k: got["d " + k] for k in C.BIL_KEYS})
        res[matmul] = C.pass_fractions(obs, ref, mag, dout.shape[0], R, factor)
        print(f"[head-bf16] passes matmul={matmul} {C.case_id(c)}: " + " ".join(f"{k}={v[0]:.3g} ({v[1]:.2f})" for k, v in res[matmul].items()))
    bad = {k: v for k, v in res[1].items() if not v[0] <= 1.0}
    assert not bad, f"bf16 passes past the derived bound: {bad}"
    assert all(res[0][k][1] > 0.5 for k in C.separating(R)), f"the fp32 head must break the bound where it separates: {res[0]}"


@pytest.mark.parametrize("case", PASS_CASES[:5] + [(B, N, 97, 3, nv) for B, N, nv in RAGGED], ids=_id)
def test_whole_head_against_the_float64_definition(gpu_device, case):
    """Logits and every gradient, C ABI and classifier_head (bit-equal to each other), against the per-document float64 definition;
    on a ragged batch the padding slots hold exactly what the fp32 head leaves there (zeros) and a NaN cotangent on padding pairs
    reaches nothing."""
    B, N, R, nf, nv = case
    c, ref = C.case_and_ref(B, N, R, nv=nv, nf=nf)
    cot = c.cot
    if c.ragged:
        cot = c.cot.clone()
        cot[~c.pair] = C.NAN
    got, _ = C.run_abi(c, gpu_device, 1, cot=cot)
    res = C.e2e_fractions(got, ref)
    print(f"[head-bf16] end to end {C.case_id(c)}: " + " ".join(f"{k}={v:.4f}" for k, v in res.items()))
    assert max(res.values()) <= 1.0, res
    via_python = C.run_fn(c, gpu_device, "bf16", cot=cot)
    for k, v in got.items():
        assert torch.equal(v, via_python[k]), f"{k}: classifier_head(matmul='bf16') is not the C ABI's result"
    if c.ragged:
        fp32, _ = C.run_abi(c, gpu_device, 0, cot=cot)
        pad_e, pad_p = ~c.real.to(gpu_device), ~c.pair.to(gpu_device)
        assert torch.equal(got["logits"][pad_p], fp32["logits"][pad_p]) and float(got["logits"][pad_p].abs().sum()) == 0.0
        for k in range(c.nf):
            assert float(got[f"d f{k}"][pad_e].abs().sum()) == 0.0
    assert float(got["d ner_emb.weight"][0].abs().sum()) == 0.0


def test_two_runs_and_a_captured_replay_are_bit_equal(gpu_device):
    """Eager twice; forward + backward captured in a graph replays bit-equal to eager, and again after n_valid.copy_(other)."""
    dev = gpu_device
    c = C.make_case(3, 12, 97, nv=(12, 7, 0))
    other = C.make_case(3, 12, 97, nv=(5, 12, 9))
    first, second = C.run_fn(c, dev, "bf16"), C.run_fn(c, dev, "bf16")
    for k in first:
        assert torch.equal(first[k], second[k]), k
    c2 = C.make_case(3, 12, 97, nv=(12, 7, 0))
    c2.nv = other.nv
    want_other = C.run_fn(c2, dev, "bf16")

    from gcgcn_amd import functional as F_, params as P_
    dims = (c.Hd, c.nf, c.Pt, c.Pr, c.R)
    flat = torch.zeros(P_.head_layout(*dims)[-1])
    P_.pack_head(c.sd, *dims, flat)
    flat = flat.to(dev).requires_grad_()
    fg = [f.to(dev).requires_grad_() for f in c.feats]
    ner, dis = c.sd["ner_emb.weight"].to(dev).requires_grad_(), c.sd["dis_embed.weight"].to(dev).requires_grad_()
    ntype, rel, nvd, cot = c.ntype.to(dev), c.rel.to(dev), c.nv.to(dev), c.cot.to(dev)
    leaves = [flat, ner, dis] + fg
    old = F_.check_ids
    F_.check_ids = False

    def step():
        out = F_.classifier_head(fg, ntype, rel, ner, dis, flat, c.R, nvd, c.dis_plus, matmul="bf16")
        return out, torch.autograd.grad(out, leaves, cot)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, grads = step()
        for want, nv in ((first, c.nv), (want_other, other.nv)):
            nvd.copy_(nv.to(dev))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want["logits"])
            gflat = P_.unpack_head(grads[0], *dims)
            for k in C.PARAM_KEYS:
                assert torch.equal(gflat[k], want["d " + k]), k
            assert torch.equal(grads[1], want["d ner_emb.weight"]) and torch.equal(grads[2], want["d dis_embed.weight"])
            for k in range(c.nf):
                assert torch.equal(grads[3 + k], want[f"d f{k}"]), k
    finally:
        F_.check_ids = old


def _launches(tag, fn):
    ms, n, w = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
    _lib.call("gcgcn_prof_start", tag, 64)
    try:
        fn()
    finally:
        _lib.call("gcgcn_prof_stop", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w))
    return n.value


@pytest.mark.parametrize("nv", [None, (12, 7, 0)], ids=["dense", "ragged"])
def test_default_is_untouched(gpu_device, nv):
    """matmul="fp32" and no argument: bit-equal logits and gradients, and not one launch of the new file; "bf16" launches them (three
    passes and the weight gradients with its reduce) and none of the fp32 bilinear kernels."""
    c = C.make_case(3, 12, 97, nv=nv)
    plain, named = C.run_fn(c, gpu_device), C.run_fn(c, gpu_device, "fp32")
    for k in plain:
        assert torch.equal(plain[k], named[k]), k
    assert _launches(b"head_bf16", lambda: C.run_fn(c, gpu_device)) == 0
    assert _launches(b"head_bf16", lambda: C.run_fn(c, gpu_device, "fp32")) == 0
    assert _launches(b"head_bilinear", lambda: C.run_fn(c, gpu_device)) >= 4
    assert _launches(b"head_bf16_bilinear", lambda: C.run_fn(c, gpu_device, "bf16")) == 4
    assert _launches(b"head_bf16_reduce", lambda: C.run_fn(c, gpu_device, "bf16")) == 1     # 432 pair slots: K split over two
    assert _launches(b"head_bilinear", lambda: C.run_fn(c, gpu_device, "bf16")) == 0


def test_model_with_the_bf16_head(gpu_device):
    """GCGCN_glove at the model_step_c1 fixture's sizes, eval mode: config.head_matmul = "bf16" against the default model within the
    end-to-end bound; strict loads both ways."""
    from gcgcn_amd import models as M
    from lstm_cases import Cfg, doc_tensors, load_model
    g, sd, plain = load_model(gpu_device)
    cfg = Cfg(g["meta"]["vocab"])
    cfg.head_matmul = "bf16"
    opted = M.GCGCN_glove(cfg).to(gpu_device).eval()
    assert opted.head.matmul == "bf16" and plain.head.matmul == "fp32"
    assert list(opted.state_dict()) == list(plain.state_dict())
    for dst, src in ((opted, plain), (plain, opted)):
        res = dst.load_state_dict(src.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    cfg.head_matmul = "half"
    with pytest.raises(ValueError, match="matmul must be 'fp32' or 'bf16'"):
        M.GCGCN_glove(cfg)
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(g["meta"]["docs"])]
    batch = {k: torch.stack([d[k] for d in docs]) for k in docs[0]}
    with torch.no_grad():
        want, got = plain(**batch), opted(**batch)
    fr = C.e2e_fractions({"logits": got}, {"logits": want.cpu()})["logits"]
    print(f"[head-bf16] model logits, bf16 head against the default: {fr:.3f} of the bound")
    assert fr <= 1.0 and not torch.equal(got, want)
