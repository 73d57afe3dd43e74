"""FusedAdam beyond plain Adam on the device (gcopt_adamw_step / gcopt_adamw_step_dev, include/gcgcn_optim.h): weight decay (L2
and decoupled), amsgrad, maximize, bias correction off, one clipping norm over all parameter groups, capture, checkpoints to and from torch's AdamW.
Cases, float64 CPU references and the bound (ATOL, RTOL, derived there from torch's own float32 error): tests/optim_cases.py."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib
from gcgcn_amd.bert import BertConfig, BertModel
from gcgcn_amd.optim import FusedAdam, GraphedTrainStep

import optim_cases as C

pytestmark = pytest.mark.gpu


def _within(got, ref, what, keys=("param",) + C.STATE_KEYS):
    worst = C.worst_fraction(got, ref, keys=keys)
    print(f"{what}: {worst:.4f} of the bound ({C.ATOL:g}, {C.RTOL:g})")
    assert got["step"] == ref["step"], what
    assert worst <= 1.0, f"{what}: {worst:.3f} of the bound"


def _launches(tag, fn):
    ms, n, w = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
    _lib.call("gcgcn_prof_start", tag, 64)
    try:
        fn()
    finally:
        _lib.call("gcgcn_prof_stop", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w))
    return n.value


@pytest.mark.parametrize("capturable", [False, True], ids=["default", "capturable"])
@pytest.mark.parametrize("maximize", [False, True], ids=["", "maximize"])
@pytest.mark.parametrize("amsgrad", [False, True], ids=["", "amsgrad"])
@pytest.mark.parametrize("decay", ["none", "l2", "decoupled"])
def test_accuracy_against_float64_torch(gpu_device, decay, amsgrad, maximize, capturable):
    """Five steps over the ten tensors of the case list: parameters, exp_avg, exp_avg_sq and max_exp_avg_sq within the bound of
    torch.optim.Adam's float64 CPU run; two runs from the same values land on the same bits."""
    h = C.hyper(decay, amsgrad, maximize)
    runs = [C.run(lambda ps: FusedAdam(ps, capturable=capturable, **h), amsgrad, gpu_device) for _ in range(2)]
    opt = runs[0][1]
    assert opt.route() == ("adam" if (decay, amsgrad, maximize) == ("none", False, False) else "adamw")
    got = C.collect(*runs[0])
    _within(got, C.torch_reference(decay, amsgrad, maximize), f"{decay} amsgrad={amsgrad} maximize={maximize} capturable={capturable}")
    assert all((v is not None) == amsgrad for v in got["max_exp_avg_sq"])
    again = C.collect(*runs[1])
    for k in ("param",) + C.STATE_KEYS:
        assert all(torch.equal(a, b) for a, b in zip(got[k], again[k]) if a is not None), k


@pytest.mark.parametrize("capturable", [False, True], ids=["default", "capturable"])
def test_no_bias_correction(gpu_device, capturable):
    """bias_correction=False with decoupled decay (BertAdam's update; tests/test_optim_decay_cpu.py holds the restatement against
    BertAdam's formula), and with L2 decay and amsgrad."""
    for decay, amsgrad in (("decoupled", False), ("l2", True)):
        h = C.hyper(decay, amsgrad, bias_correction=False)
        got = C.collect(*C.run(lambda ps: FusedAdam(ps, capturable=capturable, **h), amsgrad, gpu_device))
        _within(got, C.restatement(*C.draw(amsgrad), h), f"no bias correction, {decay}, amsgrad={amsgrad}, capturable={capturable}")
        with_bc = C.torch_reference(decay, amsgrad)
        assert C.outside_fraction(got, with_bc) >= 0.5                      # and it is not the corrected update


def _clip_run(dev, scope):
    base, _ = C.draw(False, C.SEED + 1)
    params = C.make_params(base, dev)
    opt = FusedAdam(C.clip_groups(params), decoupled_weight_decay=True, capturable=True, max_grad_norm=C.CLIP_MAX_NORM, clip_scope=scope)
    norms = []
    for s in range(C.STEPS):
        grads, scales = C.clip_grads(s)
        for p, g, c in zip(params, grads, scales):
            p.grad = g.to(dev) * c
        opt.step()
        norms.append(opt.last_grad_norm.clone())
    return params, opt, norms


def test_two_groups_one_clipping_norm(gpu_device):
    """Decay and no-decay groups with different lr, clip_scope="global", the clip active in every step: clip_grad_norm_ over ALL
    parameters, then AdamW, in float64.  The norm: an element's path to the sum of squares passes at most 22 fp32 roundings of
    positive terms (its square, 3 adds in the lane, 8 in the workgroup's tree, 1 + 8 in the tick, its own input rounding), each
    2^-24 relative, and the root halves the total: 16 * 2^-24 relative.  Clipping each group by its own norm is another
    optimiser: the same data under clip_scope="group" is outside the bound on more than half of the elements."""
    ref, ref_norms = C.clip_reference("global")
    params, opt, norms = _clip_run(gpu_device, "global")
    assert opt.route() == "adamw"
    for got, want in zip(norms, ref_norms):
        assert got.dim() == 0 and got.is_cuda and want > 100 * C.CLIP_MAX_NORM
        assert abs(got.item() - want) <= 16 * 2.0 ** -24 * want, (got.item(), want)
    _within(C.collect(params, opt), ref, "two groups, global clipping", keys=("param", "exp_avg", "exp_avg_sq"))
    # the same run again: the norm and the parameters are bit-reproducible
    params2, _, norms2 = _clip_run(gpu_device, "global")
    assert all(torch.equal(a, b) for a, b in zip(norms, norms2)) and all(torch.equal(a, b) for a, b in zip(params, params2))
    # per-group clipping: its own float64 reference, and outside the bound of the global one
    pg, og, ng = _clip_run(gpu_device, "group")
    ref_g, ref_norms_g = C.clip_reference("group")
    assert ng[-1].shape == (2,) and all(abs(ng[-1][i].item() - ref_norms_g[-1][i]) <= 16 * 2.0 ** -24 * ref_norms_g[-1][i] for i in range(2))
    _within(C.collect(pg, og), ref_g, "two groups, per-group clipping", keys=("param", "exp_avg", "exp_avg_sq"))
    share = C.outside_fraction(C.collect(pg, og), ref)
    print(f"clip_scope='group' against the global reference: {share:.3f} of the elements outside the bound")
    assert share >= 0.5


def test_launch_counts(gpu_device):
    """Three launches for two groups with global clipping, two without clipping, one in the default form whatever the number of
    groups; plain groups launch none of the new kernels."""
    base, grads = C.draw(False)

    def count(tag, **kw):
        params = C.make_params(base, gpu_device)
        groups = [{"params": params[0::2], "weight_decay": C.WD}, {"params": params[1::2], "weight_decay": 0.0, "lr": 1e-3}]
        opt = FusedAdam(groups, lr=C.LR, **kw)
        C.set_grads(params, grads[0])
        opt.step()                                                          # state, device scalars, workspace
        return _launches(tag, opt.step)

    assert count(b"adamw", decoupled_weight_decay=True, capturable=True, max_grad_norm=1.0, clip_scope="global") == 3
    assert count(b"adamw", decoupled_weight_decay=True, capturable=True, clip_scope="global") == 2
    assert count(b"adamw", decoupled_weight_decay=True) == 1
    assert count(b"adam_step", decoupled_weight_decay=True, capturable=True, max_grad_norm=1.0, clip_scope="global") == 0
    params = C.make_params(base, gpu_device)
    plain = FusedAdam([{"params": params[0::2]}, {"params": params[1::2], "lr": 1e-3}], lr=C.LR, capturable=True, max_grad_norm=1.0)
    C.set_grads(params, grads[0])
    plain.step()
    assert _launches(b"adamw", plain.step) == 0 and _launches(b"adam_step_dev", plain.step) == 2


def test_plain_groups_make_the_calls_they_made(gpu_device):
    """Plain Adam groups through FusedAdam against the same steps driven through gcgcn_adam_step / gcgcn_adam_step_dev directly,
    from tables built here: bitwise equal parameters and moments."""
    base, grads = C.draw(False)
    for capturable in (False, True):
        pa, pb = C.make_params(base, gpu_device), C.make_params(base, gpu_device)
        oa = FusedAdam(pa, lr=C.LR, capturable=capturable, max_grad_norm=1.0 if capturable else None)
        assert oa.route() == "adam"
        m, v = [torch.zeros_like(p) for p in pb], [torch.zeros_like(p) for p in pb]
        t = [0] * len(pb)
        steps = [torch.zeros((), device=gpu_device) for _ in pb]
        lr = torch.tensor(C.LR, dtype=torch.float32, device=gpu_device)
        norm = torch.zeros((), device=gpu_device)
        for s in range(C.STEPS):
            C.set_grads(pa, grads[s])
            C.set_grads(pb, grads[s])
            oa.step()
            rows, blocks = [], 0
            for i, p in enumerate(pb):
                if p.grad is None or (p.numel() == 0 and not capturable):
                    continue
                t[i] += 1
                last = steps[i].data_ptr() if capturable else int(np.array(
                    [C.LR / (1.0 - 0.9 ** t[i]), 1.0 / math.sqrt(1.0 - 0.999 ** t[i])], dtype=np.float32).view(np.int64)[0])
                rows.append((p.data_ptr(), p.grad.data_ptr(), m[i].data_ptr(), v[i].data_ptr(), p.numel(), blocks, last))
                blocks += (p.numel() + 1023) // 1024
            tab = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(gpu_device)
            if capturable:
                ws = torch.empty(_lib.lib().gcgcn_adam_ws_bytes(len(rows), blocks), dtype=torch.uint8, device=gpu_device)
                _lib.call("gcgcn_adam_step_dev", len(rows), tab.data_ptr(), blocks, 0.9, 0.999, 1e-8, lr.data_ptr(), 1.0, ws.data_ptr(),
                          ws.numel(), norm.data_ptr(), torch.cuda.current_stream().cuda_stream)
            else:
                _lib.call("gcgcn_adam_step", len(rows), tab.data_ptr(), blocks, 0.9, 0.999, 1e-8, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert torch.equal(a.detach(), b.detach()), (capturable, i)
            assert torch.equal(oa.state[a]["exp_avg"], m[i]) and torch.equal(oa.state[a]["exp_avg_sq"], v[i]), (capturable, i)
        if capturable:
            assert torch.equal(oa.last_grad_norm, norm)


def _tiny_bert(dev, seed):
    torch.manual_seed(seed)
    cfg = BertConfig(vocab_size=40, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128, max_position_embeddings=16)
    model = BertModel(cfg, impl="hip").to(dev).eval()
    for t in (model.embeddings.word_embeddings, model.embeddings.position_embeddings, model.embeddings.token_type_embeddings):
        t.weight.requires_grad_(False)       # torch's embedding backward adds with atomics: not a bitwise yardstick
    return model


def test_graphed_train_step_on_a_tiny_bert(gpu_device):
    """GraphedTrainStep over a 1-layer BertModel(impl="hip") (hidden 64, one head, T = 16, B = 2) with bert_param_groups, decoupled
    decay and one clipping norm: three replays against three eager steps of a twin, bitwise; the no-decay group's lr changes before
    the third through sync_lr(), without a new capture."""
    dev = gpu_device
    mg, me = _tiny_bert(dev, 3), _tiny_bert(dev, 3)
    gen = torch.Generator().manual_seed(4)
    ids = [torch.randperm(40, generator=gen)[:32].view(2, 16).to(dev) for _ in range(3)]
    dy = torch.randn(2, 16, 64, generator=gen).to(dev)

    def step_of(model):
        def step_fn(input_ids):
            last, pooled = model(input_ids, output_all_encoded_layers=False)
            return (last * dy).sum() + pooled.sum()
        return step_fn

    def make(model):
        groups = gcgcn_amd.bert_param_groups(model, 0.1)
        assert len(groups[0]["params"]) == 7 and len(groups[1]["params"]) == 13
        return FusedAdam(groups, lr=1e-3, decoupled_weight_decay=True, capturable=True, max_grad_norm=0.5, clip_scope="global")

    og, oe = make(mg), make(me)
    train = GraphedTrainStep(step_of(mg), og, {"input_ids": ids[0].clone()}, warmup=2)
    assert len(og._graph_tables) == 1
    step_e = step_of(me)
    for k in range(3):
        if k == 2:
            og.param_groups[1]["lr"] = oe.param_groups[1]["lr"] = 4e-3
        loss_g = train(input_ids=ids[k])
        for p in me.parameters():
            p.grad = None
        loss_e = step_e(ids[k])
        loss_e.backward()
        oe.step()
        assert torch.equal(loss_g.detach(), loss_e.detach()), k
        assert torch.equal(og.last_grad_norm, oe.last_grad_norm) and og.last_grad_norm.item() > 0.5, k      # the clip is active
    torch.cuda.synchronize()
    moved = 0
    for (n, a), b in zip(mg.named_parameters(), me.parameters()):
        assert torch.equal(a, b), n
        if a.requires_grad:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(og.state[a][key], oe.state[b][key]), (n, key)
            assert og.state[a]["step"].item() == 3.0
            moved += 1
    assert moved == 20
    # the eager twin stepped with the new lr, so equality above means the replay did too; the device scalars say the same
    assert og._dev[1]["lr"].item() == pytest.approx(4e-3) and og._dev[0]["lr"].item() == pytest.approx(1e-3)


def test_first_step_inside_a_capture_raises(gpu_device, monkeypatch):
    """As in the plain capturable form.  No stream is put into capture for this: the optimiser asks torch whether one is."""
    base, grads = C.draw(False)
    params = C.make_params(base, gpu_device)
    opt = FusedAdam(params, lr=C.LR, weight_decay=C.WD, capturable=True)
    C.set_grads(params, grads[0])
    opt.sync_lr()                            # the device-side lr exists; what is missing is the parameters' state
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="first step"):
        opt.step()


def test_capture_needs_its_warm_up(gpu_device, monkeypatch):
    """The other things a captured step must find in place, each asked for by name: amsgrad's running maximum, the norm tensor,
    the pinned buffer that the captured call will own.  The capture is pretended, as above."""
    base, grads = C.draw(False)

    def warm(**kw):
        params = C.make_params(base, gpu_device)
        opt = FusedAdam(params, lr=C.LR, weight_decay=C.WD, capturable=True, max_grad_norm=1.0, **kw)
        C.set_grads(params, grads[0])
        opt.step()
        return params, opt

    params, opt = warm()
    opt.param_groups[0]["amsgrad"] = True                 # switched on after the warm-up: max_exp_avg_sq does not exist yet
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="max_exp_avg_sq must exist before the capture"):
            opt.step()
    opt.step()                                            # outside a capture it is created, as zeros
    assert all("max_exp_avg_sq" in opt.state[p] for p in params)
    params, opt = warm()
    opt._norms = None
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="warm up with one step"):
            opt.step()
    params, opt = warm()
    assert opt._spare is not None
    opt._spare = None                                     # as after a first capture: the buffer went to that graph
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="outside the capture first"):
            opt.step()
    assert opt._graph_tables == []


@pytest.mark.parametrize("capturable", [False, True], ids=["default", "capturable"])
def test_an_empty_group_changes_nothing(gpu_device, capturable):
    """Parameter groups without parameters (torch accepts them; frozen models produce them) and a group whose parameters have no
    gradient: no record of theirs reaches the kernels, and the step is bit for bit the step without them."""
    base, grads = C.draw(False)
    kw = dict(lr=C.LR, decoupled_weight_decay=True, capturable=capturable)
    if capturable:
        kw.update(max_grad_norm=0.5, clip_scope="global")
    pa, pb = C.make_params(base, gpu_device), C.make_params(base, gpu_device)
    idle = torch.zeros(5, device=gpu_device, requires_grad=True)            # never gets a gradient
    oa = FusedAdam([{"params": [], "weight_decay": 0.3, "lr": 0.5}, {"params": pa, "weight_decay": C.WD}, {"params": [idle], "lr": 0.25},
                    {"params": []}], **kw)
    ob = FusedAdam([{"params": pb, "weight_decay": C.WD}], **kw)
    for s in range(3):
        C.set_grads(pa, grads[s])
        C.set_grads(pb, grads[s])
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a.detach(), b.detach()), i
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[a][key], ob.state[b][key]), (i, key)
    assert not idle.any() and not oa.state.get(idle)
    if capturable:
        assert oa.last_grad_norm.dim() == 0 and torch.equal(oa.last_grad_norm, ob.last_grad_norm) and oa.last_grad_norm.item() > 0.5
        assert 0 not in oa._dev and 3 not in oa._dev                        # a group without parameters has no device-side lr at all
    only_empty = FusedAdam([{"params": [], "weight_decay": 0.1}], **kw)
    only_empty.step()                                                       # nothing to do, nothing launched


def _adamw_pair(dev, fused_first):
    """Two steps under one optimiser, its checkpoint into the other, two more steps there; against the first one continuing."""
    base, grads = C.draw(True)
    kw = dict(lr=C.LR, betas=C.AMS_BETAS, weight_decay=C.WD, amsgrad=True, capturable=True)
    mk_torch = lambda ps: torch.optim.AdamW(ps, foreach=False, **kw)
    mk_fused = lambda ps: FusedAdam(ps, decoupled_weight_decay=True, **kw)
    first, second = (mk_fused, mk_torch) if fused_first else (mk_torch, mk_fused)
    pa, pb = C.make_params(base, dev), C.make_params(base, dev)
    oa, ob = first(pa), first(pb)
    for s in (0, 1):
        for ps, o in ((pa, oa), (pb, ob)):
            C.set_grads(ps, grads[s])
            o.step()
    oc = second(pb)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    g = oc.param_groups[0]
    assert g["decoupled_weight_decay"] is True and g["amsgrad"] is True and g["weight_decay"] == C.WD and g["capturable"] is True
    for s in (2, 3):
        C.set_grads(pa, grads[s])
        C.set_grads(pb, grads[s])
        oa.step()
        oc.step()
    return C.collect(pb, oc), C.collect(pa, oa)


def test_checkpoint_from_torch_adamw(gpu_device):
    got, want = _adamw_pair(gpu_device, fused_first=False)
    _within(got, want, "torch.optim.AdamW(capturable=True) -> FusedAdam, two steps on")


def test_checkpoint_into_torch_adamw(gpu_device):
    got, want = _adamw_pair(gpu_device, fused_first=True)
    _within(got, want, "FusedAdam -> torch.optim.AdamW(capturable=True), two steps on")


def test_a_decayed_torch_checkpoint_steps(gpu_device):
    """torch.optim.Adam(weight_decay) -> a default-form FusedAdam built for weight decay: the checkpoint's hyper-parameters replace
    the constructor's and the steps go on as torch's would.  A FusedAdam built as plain Adam still refuses such a checkpoint."""
    base, grads = C.draw(False)
    pa, pb = C.make_params(base, gpu_device), C.make_params(base, gpu_device)
    oa = torch.optim.Adam(pa, foreach=False, **C.hyper("l2"))
    ob = FusedAdam(pb, lr=1.0, weight_decay=0.5)
    plain = FusedAdam(C.make_params(base, gpu_device), lr=1.0)
    for s in range(C.STEPS):
        C.set_grads(pa, grads[s])
        C.set_grads(pb, grads[s])
        oa.step()
        if s == 1:
            for a, b in zip(pa, pb):
                b.data.copy_(a.data)
            ob.load_state_dict(copy.deepcopy(oa.state_dict()))
            assert ob.param_groups[0]["lr"] == C.LR and ob.param_groups[0]["weight_decay"] == C.WD
            plain.load_state_dict(copy.deepcopy(oa.state_dict()))
            C.set_grads(plain.param_groups[0]["params"], grads[s])
            with pytest.raises(RuntimeError, match="weight_decay"):
                plain.step()
        if s >= 2:
            ob.step()
    _within(C.collect(pb, ob), C.torch_reference("l2"), "torch.optim.Adam(weight_decay) -> FusedAdam", keys=("param", "exp_avg", "exp_avg_sq"))


def test_non_finite_gradient(gpu_device):
    """One NaN gradient element in one group: the norm is NaN, so is the one coefficient, and every parameter of BOTH groups takes
    it, as torch's clip_grad_norm_(error_if_nonfinite=False) followed by a step would leave them."""
    base, _ = C.draw(False, C.SEED + 1)
    params = C.make_params(base, gpu_device)
    opt = FusedAdam(C.clip_groups(params), decoupled_weight_decay=True, capturable=True, max_grad_norm=C.CLIP_MAX_NORM, clip_scope="global")
    grads, _ = C.clip_grads(0)
    C.set_grads(params, grads)
    opt.step()
    assert torch.isfinite(opt.last_grad_norm) and all(torch.isfinite(p).all() for p in params)
    params[3].grad[7] = float("nan")
    opt.step()
    assert torch.isnan(opt.last_grad_norm)
    assert all(torch.isnan(p).all() for p in params)
