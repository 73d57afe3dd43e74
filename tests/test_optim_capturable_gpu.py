"""FusedAdam(capturable=True): the optimiser step whose hipGraph replay TRAINS (gcgcn_adam_step_dev: step counters and the
learning rate on the device, gradient clipping in the same call), and gcgcn_amd.GraphedTrainStep, the whole training step as one
graph.  References: torch.optim.Adam(capturable=True) (+ torch.nn.utils.clip_grad_norm_) and the default FusedAdam, at the
tolerances of tests/test_model_gpu.py::test_fused_adam_is_torch_adam; an eager run of the same kernels, bit for bit."""
import copy

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd.optim import FusedAdam, GraphedTrainStep

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 100), (7,), (1, 1), (513, 3), (4096,), (33, 31)]     # test_fused_adam_is_torch_adam's, + an unaligned view of 2000
LR = 1e-2


def _base(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return gen, [torch.randn(*s, generator=gen) for s in SHAPES] + [torch.randn(2000, generator=gen)]


def _params(base, dev):
    """Fresh leaf parameters holding `base`; the last one is a view that starts 4 bytes past a 16-byte boundary (scalar path)."""
    out = [b.clone().to(dev).requires_grad_() for b in base[:-1]]
    buf = torch.empty(base[-1].numel() + 1, device=dev)
    buf[1:] = base[-1].to(dev)
    out.append(buf[1:].requires_grad_())
    assert out[-1].data_ptr() % 16 == 4
    return out


def _grad_steps(gen, base, steps, scale=None, skip=((1, 1), (1, 2))):
    """Per step a list of gradients (None: parameter skipped in that step); tensor i scaled by 10^(i-3) as in the torch test."""
    out = []
    for s in range(steps):
        out.append([None if (i, s) in skip else torch.randn(b.shape, generator=gen) * (10.0 ** (i - 3) if scale is None else scale[s])
                    for i, b in enumerate(base)])
    return out


def _set_grads(params, grads, dev):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.to(dev).clone()


def _close(pa, oa, pb, ob, what):
    """test_fused_adam_is_torch_adam's tolerances."""
    for i, (a, b) in enumerate(zip(pa, pb)):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-6, msg=lambda m: f"{what}, parameter {i}: {m}")
        sa, sb = oa.state.get(a), ob.state.get(b)
        assert bool(sa) == bool(sb)
        if not sa:
            continue
        assert float(sa["step"]) == float(sb["step"]), f"{what}, parameter {i}: step {float(sa['step'])} != {float(sb['step'])}"
        torch.testing.assert_close(sa["exp_avg"], sb["exp_avg"], rtol=1e-5, atol=1e-9, msg=lambda m: f"{what}, exp_avg {i}: {m}")
        torch.testing.assert_close(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-5, atol=1e-12, msg=lambda m: f"{what}, exp_avg_sq {i}: {m}")


def _equal(pa, oa, pb, ob, what):
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a.detach(), b.detach()), f"{what}: parameter {i} is not bitwise equal"
        sa, sb = oa.state.get(a), ob.state.get(b)
        assert bool(sa) == bool(sb)
        for k in (sa or {}):
            assert torch.equal(sa[k], sb[k]), f"{what}: {k} of parameter {i} is not bitwise equal"


def test_capturable_eager_is_torch_capturable_and_default_fused_adam(gpu_device):
    gen, base = _base()
    pa, pb, pc = (_params(base, gpu_device) for _ in range(3))
    oa = FusedAdam(pa, lr=LR, capturable=True)
    ob = torch.optim.Adam(pb, lr=LR, capturable=True)
    oc = FusedAdam(pc, lr=LR)
    for key in ("capturable", "max_grad_norm", "weight_decay", "amsgrad", "maximize"):
        assert key in oa.state_dict()["param_groups"][0] and key in oc.state_dict()["param_groups"][0]
    assert oa.param_groups[0]["capturable"] is True and oc.param_groups[0]["capturable"] is False
    for grads in _grad_steps(gen, base, 5):
        for ps, o in ((pa, oa), (pb, ob), (pc, oc)):
            _set_grads(ps, grads, gpu_device)
            o.step()
    _close(pa, oa, pb, ob, "against torch.optim.Adam(capturable=True)")
    _close(pa, oa, pc, oc, "against the default FusedAdam")
    for i, p in enumerate(pa):
        st = oa.state[p]["step"]
        assert torch.is_tensor(st) and st.is_cuda and st.dtype == torch.float32 and st.dim() == 0       # torch's capturable format
        assert st.item() == (3.0 if i == 1 else 5.0)
    assert [int(oc.state[p]["step"]) for p in pc] == [5, 3, 5, 5, 5, 5, 5]
    with pytest.raises(ValueError, match="capturable"):
        FusedAdam(pc, lr=LR, max_grad_norm=1.0)
    od = FusedAdam(pc, lr=LR, capturable=True)
    od.param_groups[0]["weight_decay"] = 0.01
    with pytest.raises(RuntimeError, match="weight_decay"):
        od.step()


def _captured_step(opt, params, base, dev):
    """One opt.step() over static gradient buffers in a hipGraph.  The warm-up step that has to precede the capture (state and
    device scalars must exist outside the graph) is undone in place: parameters back to `base`, moments and counters to zero."""
    static = [torch.zeros_like(p) for p in params]
    for p, g in zip(params, static):
        p.grad = g
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    with torch.no_grad():
        for p, b in zip(params, base):
            p.copy_(b.to(dev))
            for v in opt.state[p].values():
                v.zero_()
    return graph, static


def _replay_against_eager(dev, lr_change=None, max_grad_norm=None):
    gen, base = _base(2)
    pg, pe, pn = (_params(base, dev) for _ in range(3))
    og = FusedAdam(pg, lr=LR, capturable=True, max_grad_norm=max_grad_norm)        # replayed
    oe = FusedAdam(pe, lr=LR, capturable=True, max_grad_norm=max_grad_norm)        # the same kernels, launched eagerly
    on = FusedAdam(pn, lr=LR)                                                      # the default form
    graph, static = _captured_step(og, pg, base, dev)
    assert len(og._graph_tables) == 1 and all(og._graph_tables[0].data_ptr() != s[0].data_ptr() for s in og._ring)
    table = og._graph_tables[0].clone()
    for k, grads in enumerate(_grad_steps(gen, base, 6, skip=())):
        if lr_change is not None and k == 3:
            for o in (og, oe, on):
                o.param_groups[0]["lr"] = lr_change
            og.sync_lr()                                  # a stream-ordered fill of the device scalar: the graph is not captured again
        for s, g in zip(static, grads):
            s.copy_(g.to(dev))
        graph.replay()
        for ps, o in ((pe, oe), (pn, on)):
            _set_grads(ps, grads, dev)
            o.step()
    torch.cuda.synchronize()
    assert torch.equal(og._graph_tables[0], table)        # the table the replays read is never rewritten
    _equal(pg, og, pe, oe, "replay against the eager capturable step")
    if max_grad_norm is None:
        _close(pg, og, pn, on, "replay against the default FusedAdam")
    assert all(og.state[p]["step"].item() == 6.0 for p in pg)
    if max_grad_norm is not None:
        assert torch.equal(og.last_grad_norm, oe.last_grad_norm)
    return pg, og


def test_step_counter_moves_under_replay(gpu_device):
    """A frozen t (the default form captured at t = 1) applies 10 x lr instead of 2.1 x lr at the sixth step: far outside 1e-5."""
    _replay_against_eager(gpu_device)


def test_learning_rate_changes_without_recapture(gpu_device):
    _replay_against_eager(gpu_device, lr_change=2.5e-3)


def test_clipping_under_replay(gpu_device):
    """Three launches in the graph; the clip is active in every step (|g| ~ 4e4) and the norm the replay leaves is the eager one's."""
    _, og = _replay_against_eager(gpu_device, max_grad_norm=1.0)
    assert og.last_grad_norm.item() > 1e3


def _clip_run(dev, max_norm, scales):
    """[inactive, active, inactive, active] steps of FusedAdam(max_grad_norm) against clip_grad_norm_ + torch's capturable Adam;
    before each inactive step a twin without clipping takes over parameters and state and must land on the same bits."""
    gen, base = _base(3)
    pa, pb = _params(base, dev), _params(base, dev)
    oa = FusedAdam(pa, lr=LR, capturable=True, max_grad_norm=max_norm)
    ob = torch.optim.Adam(pb, lr=LR, capturable=True)
    norms, active = [], []
    for s, grads in enumerate(_grad_steps(gen, base, len(scales), scale=scales, skip=((1, 1),))):
        twin = None
        if s in (0, 2):
            pt = _params([p.detach().cpu() for p in pa], dev)
            twin = FusedAdam(pt, lr=LR, capturable=True)
            if s:
                twin.load_state_dict(copy.deepcopy(oa.state_dict()))
                assert twin.param_groups[0]["max_grad_norm"] == max_norm      # a checkpoint carries it ...
                twin.param_groups[0]["max_grad_norm"] = None                  # ... and this twin drops it
            _set_grads(pt, grads, dev)
            twin.step()
        _set_grads(pa, grads, dev)
        _set_grads(pb, grads, dev)
        kept = [p.grad.clone() for p in pa if p.grad is not None]
        oa.step()
        want = torch.nn.utils.clip_grad_norm_(pb, max_norm)
        ob.step()
        assert all(torch.equal(k, p.grad) for k, p in zip(kept, [p for p in pa if p.grad is not None]))   # .grad is NOT modified
        got = oa.last_grad_norm
        assert got.is_cuda and got.dim() == 0
        torch.testing.assert_close(got, want, rtol=1e-5, atol=0.0)
        norms.append(got.clone())
        active.append(bool(want.item() > max_norm))
        if twin is not None:
            _equal(pa, oa, pt, twin, f"step {s} (clip inactive) against max_grad_norm=None")
    assert active == [False, True, False, True]
    _close(pa, oa, pb, ob, "against clip_grad_norm_ + torch.optim.Adam(capturable=True)")
    return norms, [p.detach().clone() for p in pa]


def test_clipping_is_clip_grad_norm(gpu_device):
    # |g| ~ scale * sqrt(108 666 elements) = 330 * scale
    n1, p1 = _clip_run(gpu_device, 1.0, [1e-4, 1e-1, 1e-5, 3e-2])
    n2, p2 = _clip_run(gpu_device, 1.0, [1e-4, 1e-1, 1e-5, 3e-2])
    assert all(torch.equal(a, b) for a, b in zip(n1, n2)), "the gradient norm is not bit-reproducible"
    assert all(torch.equal(a, b) for a, b in zip(p1, p2))


def test_clipping_exact_cases(gpu_device):
    """One non-zero gradient element, the last of the unaligned view (second workgroup of the last tensor, scalar path): the norm
    is exactly 3 and coef exactly fp32(2) / fp32(3 + 1e-6), seen in the moments, which are linear and quadratic in g * coef.
    Then a table of one 1-element tensor."""
    _, base = _base(4)
    grads = [torch.zeros_like(b) for b in base]
    grads[-1][-1] = 3.0
    pa, pb = _params(base, gpu_device), _params(base, gpu_device)
    oa, ob = FusedAdam(pa, lr=LR, capturable=True, max_grad_norm=2.0), FusedAdam(pb, lr=LR, capturable=True)
    coef = np.float32(2.0) / (np.float32(3.0) + np.float32(1e-6))
    assert coef < 1
    _set_grads(pa, grads, gpu_device)
    grads[-1][-1] = float(np.float32(3.0) * coef)
    _set_grads(pb, grads, gpu_device)
    oa.step()
    ob.step()
    assert oa.last_grad_norm.item() == 3.0
    _equal(pa, oa, pb, ob, "coef")
    assert oa.state[pa[-1]]["exp_avg"][-1].item() != 0.0
    oa.param_groups[0]["max_grad_norm"] = 5.0             # inactive: coef is exactly 1
    _set_grads(pa, [g * 0 + (g != 0) * 3.0 for g in grads], gpu_device)
    _set_grads(pb, [g * 0 + (g != 0) * 3.0 for g in grads], gpu_device)
    oa.step()
    ob.step()
    assert oa.last_grad_norm.item() == 3.0
    _equal(pa, oa, pb, ob, "coef = 1")
    # a 1-element tensor alone in the table
    pc, pd = (torch.tensor([0.5], device=gpu_device, requires_grad=True) for _ in range(2))
    oc, od = FusedAdam([pc], lr=LR, capturable=True, max_grad_norm=1.0), torch.optim.Adam([pd], lr=LR, capturable=True)
    for g in (-4.0, 0.25):
        pc.grad, pd.grad = torch.tensor([g], device=gpu_device), torch.tensor([g], device=gpu_device)
        oc.step()
        want = torch.nn.utils.clip_grad_norm_([pd], 1.0)
        od.step()
        assert oc.last_grad_norm.item() == abs(g) == want.item()
    _close([pc], oc, [pd], od, "one element")
    assert oc.state[pc]["step"].item() == 2.0


def test_checkpoints_move_between_the_forms_and_torch(gpu_device):
    gen, base = _base(5)
    steps = _grad_steps(gen, base, 3, skip=((1, 1),))
    mk = {"fused capturable": lambda ps: FusedAdam(ps, lr=LR, capturable=True),
          "fused default": lambda ps: FusedAdam(ps, lr=LR),
          "torch capturable": lambda ps: torch.optim.Adam(ps, lr=LR, capturable=True)}
    for src, dst in (("fused capturable", "torch capturable"), ("torch capturable", "fused capturable"),
                     ("fused default", "fused capturable"), ("fused capturable", "fused default")):
        pa, pb = _params(base, gpu_device), _params(base, gpu_device)
        oa, ob = mk[src](pa), mk[src](pb)
        for grads in steps[:2]:
            for ps, o in ((pa, oa), (pb, ob)):
                _set_grads(ps, grads, gpu_device)
                o.step()
        oc = mk[dst](pb)                                   # pb goes on under the other optimiser, from oa's twin's checkpoint
        oc.load_state_dict(copy.deepcopy(ob.state_dict()))
        want_cap = dst != "fused default"
        assert oc.param_groups[0]["capturable"] is want_cap, f"{src} -> {dst}"
        for i, p in enumerate(pb):
            st = oc.state[p]["step"]
            if want_cap:
                assert torch.is_tensor(st) and st.is_cuda and st.dtype == torch.float32 and st.dim() == 0, f"{src} -> {dst}"
            else:
                assert isinstance(st, int), f"{src} -> {dst}"
            assert float(st) == (1.0 if i == 1 else 2.0)
        _set_grads(pa, steps[2], gpu_device)
        _set_grads(pb, steps[2], gpu_device)
        oa.step()
        oc.step()
        _close(pb, oc, pa, oa, f"{src} -> {dst}, one step on")
        assert [float(oc.state[p]["step"]) for p in pb] == [3.0, 2.0, 3.0, 3.0, 3.0, 3.0, 3.0]


def test_graphed_train_step_trains_the_model_tail(gpu_device):
    """GraphedTrainStep over GraphModelTail + pair_bce_loss (the shapes of test_tail_graph_replay_matches_eager, eval mode) against
    an eager twin with the default FusedAdam, four steps over two rotating label tensors, at the reference trainer's learning
    rate (Config.py:72, 1e-4).  Tolerances of test_model_trains_with_fused_adam for the same comparison (rtol 1e-5, atol 1e-6),
    with its exemption: tensors whose gradient is the rounding residue of an exact zero (|g| < 1e-9 throughout) move by ~lr
    or not at all depending on the summation order of the producers' fp32 atomics, in either run."""
    from gcgcn_amd import functional as F_
    from test_tail_gpu import _compact_case
    dev = gpu_device
    ctx, node, table, sen, ph, pt, nv = _compact_case(dev, B=3, N=13, S=3, T=48, seed=23)
    nv = torch.tensor([13, 5, 12], dtype=torch.int32, device=dev)
    node = node * (torch.arange(13, device=dev)[None, :] < nv[:, None]).unsqueeze(-1).float()
    B, N, _ = node.shape
    g = torch.Generator().manual_seed(5)
    ner = (torch.randn(7, 20, generator=g) * 0.3).to(dev).requires_grad_()
    for t in (ctx, node, table):                          # leaves with a gradient, as in that test: every backward kernel runs
        t.requires_grad_()
    ntype = torch.randint(0, 7, (B, N), generator=g).to(dev)
    rel = torch.randint(-10, 11, (B, N, N), generator=g).to(dev)
    labels = [(torch.rand(B, N, N, 97, generator=g) < 0.05).float().to(dev) for _ in range(2)]
    rows, pairs = F_.producer_live_counts(sen.view(torch.uint8), nv)      # capacities up front: no host read inside the step
    tail_g = gcgcn_amd.GraphModelTail().to(dev).eval()
    tail_e = gcgcn_amd.GraphModelTail().to(dev).eval()
    tail_e.load_state_dict(tail_g.state_dict())
    start = {k: v.clone() for k, v in tail_g.state_dict().items()}

    def step_of(tail):
        def step_fn(label_matrix, n_valid, **kw):
            logits = tail(n_valid=n_valid, **kw)
            return gcgcn_amd.pair_bce_loss(logits, label_matrix, n_valid=n_valid).sum() / B
        return step_fn

    inputs = dict(context_output=ctx, node_feat=node, adj_matrix=None, sen_matrix=sen, pos_matrix_h=ph, pos_matrix_t=pt, node_type=ntype,
                  node_relative_pos=rel, dis_embed_weight=table, ner_emb_weight=ner, n_valid=nv, max_live_slots=rows, max_live_pairs=pairs,
                  label_matrix=labels[0].clone())
    params_g = [p for p in tail_g.parameters() if p.requires_grad]
    params_e = [p for p in tail_e.parameters() if p.requires_grad]
    with pytest.raises(ValueError, match="capturable"):
        GraphedTrainStep(step_of(tail_g), FusedAdam(params_g, lr=1e-4), inputs)
    with pytest.raises(ValueError, match="capturable"):
        GraphedTrainStep(step_of(tail_g), torch.optim.Adam(params_g, lr=1e-4, capturable=True), inputs)
    og, oe = FusedAdam(params_g, lr=1e-4, capturable=True), FusedAdam(params_e, lr=1e-4)
    train = GraphedTrainStep(step_of(tail_g), og, inputs, warmup=2)
    torch.cuda.synchronize()
    for k, v in tail_g.state_dict().items():              # construction does not train
        assert torch.equal(v, start[k]), f"{k} moved during construction"
    stepped = [p for p in params_g if og.state.get(p)]
    assert len(stepped) >= 4 and all(og.state[p]["step"].item() == 0.0 and not og.state[p]["exp_avg"].any() for p in stepped)
    with pytest.raises(ValueError, match="shape"):
        train(label_matrix=labels[0][:, :-1])
    with pytest.raises(ValueError, match="static input"):
        train(max_live_slots=rows)

    def named_grads(tail):
        out = {}
        for name, mod in tail.named_modules():
            if name and hasattr(mod, "named_grads"):
                for k, v in mod.named_grads().items():
                    out[tail._to_model_key(f"{name}.{k}")] = v
        return out

    eager_inputs = dict(inputs)
    step_e = step_of(tail_e)
    peak = {}
    for k in range(4):
        loss_g = train(label_matrix=labels[k % 2])
        for p in params_e:
            p.grad = None
        eager_inputs["label_matrix"] = labels[k % 2]
        loss_e = step_e(**eager_inputs)
        loss_e.backward()
        for name, v in named_grads(tail_e).items():
            if v is not None:
                peak[name] = max(peak.get(name, 0.0), v.abs().max().item())
        oe.step()
        if k == 0:
            assert torch.equal(loss_g.detach(), loss_e.detach()), f"first loss {loss_g.item()} != eager {loss_e.item()}"
        print(f"step {k}: loss graph {loss_g.item():.7f} eager {loss_e.item():.7f}")
    torch.cuda.synchronize()
    assert all(og.state[p]["step"].item() == 4.0 for p in stepped)
    assert all(int(oe.state[p]["step"]) == 4 for p in params_e if oe.state.get(p))
    a, b = tail_g.state_dict(), tail_e.state_dict()
    assert set(peak) <= set(a) and len(peak) >= 25
    residue = set(k for k, v in peak.items() if v < 1e-9)
    moved = 0
    for k in a:
        print(f"{k}: max |graph - eager| = {(a[k] - b[k]).abs().max().item():.3e}, moved {(a[k] - start[k]).abs().max().item():.3e}"
              + (" (residue gradient)" if k in residue else ""))
    for k in a:
        moved += int(not torch.equal(a[k], start[k]))
        if k not in residue:
            torch.testing.assert_close(a[k], b[k], rtol=1e-5, atol=1e-6, msg=lambda m: f"{k}: {m}")
    assert moved >= len(peak) - len(residue)              # it trains: every tensor with a real gradient has moved
