"""FusedAdam beyond plain Adam, everything that needs no GPU: the bound's constants follow the project's rule, the modes can be
told apart at that bound, the float64 restatement is torch's arithmetic (and, without bias correction, BertAdam's), the route
function, the parameter groups of the BERT recipe, checkpoints' key names.  Cases and bound: tests/optim_cases.py."""
import copy
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, models as M
from gcgcn_amd.bert import BertConfig, BertModel
from gcgcn_amd.optim import FusedAdam, step_route

from conftest import GOLDEN
import optim_cases as C


def test_the_bounds_constants_follow_the_rule():
    atol, rtol, worst = C.derive_constants()
    print(f"float32 torch against float64 torch: {worst:.4f} of the bound at ({atol:g}, {rtol:g})")
    assert (atol, rtol) == (C.ATOL, C.RTOL) and worst <= 0.1


def test_the_bound_tells_the_modes_apart():
    """float64 against float64: no decay / L2 / decoupled pairwise, and amsgrad against the same draw without it, lie outside the
    bound of one another on at least half of the parameter elements."""
    for amsgrad in (False, True):
        refs = {d: C.torch_reference(d, amsgrad) for d in ("none", "l2", "decoupled")}
        for a, b in (("none", "l2"), ("none", "decoupled"), ("l2", "decoupled")):
            share = C.outside_fraction(refs[a], refs[b])
            print(f"amsgrad={amsgrad}: {a} against {b}: {share:.3f} of the elements outside the bound")
            assert share >= 0.5
    for decay in ("none", "l2", "decoupled"):
        h = dict(C.hyper(decay, True), amsgrad=False)      # the amsgrad case's betas and gradients, amsgrad off
        off = C.collect(*C.run(lambda ps: torch.optim.Adam(ps, foreach=False, **h), True, dtype=torch.float64))
        share = C.outside_fraction(C.torch_reference(decay, True), off)
        print(f"{decay}: amsgrad against amsgrad=False: {share:.3f} of the elements outside the bound")
        assert share >= 0.5


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("decay", ["none", "l2", "decoupled"])
def test_the_restatement_is_torchs_arithmetic(decay, amsgrad, maximize):
    base, grads = C.draw(amsgrad)
    mine, ref = C.restatement(base, grads, C.hyper(decay, amsgrad, maximize)), C.torch_reference(decay, amsgrad, maximize)
    assert mine["step"] == ref["step"] and ref["step"][C.LAGGING] == C.STEPS - len(C.LAG_STEPS) and ref["step"][0] == C.STEPS
    assert C.worst_fraction(mine, ref) <= 1e-3              # two float64 runs: 1e-10 of the bound in practice


def test_maximize_is_the_negated_gradient():
    base, grads = C.draw(False)
    neg = [[None if g is None else -g for g in gs] for gs in grads]
    for decay in ("none", "l2", "decoupled"):
        ref = C.torch_reference(decay, False, True)
        params = C.make_params(base, dtype=torch.float64)
        opt = torch.optim.Adam(params, foreach=False, **C.hyper(decay, False, False))
        for gs in neg:
            C.set_grads(params, gs)
            opt.step()
        got = C.collect(params, opt)
        for k in ("param", "exp_avg", "exp_avg_sq"):
            assert all(torch.equal(a, b) for a, b in zip(got[k], ref[k]) if b is not None), (decay, k)


def test_no_bias_correction_with_decoupled_decay_is_bertadam():
    """BertAdam as published (pytorch_pretrained_bert's optimization.py, schedule and clipping aside): next_m = b1 m + (1 - b1) g,
    next_v = b2 v + (1 - b2) g^2, update = next_m / (sqrt(next_v) + e) + w p, p <- p - lr update.  That is p (1 - lr w) - lr
    next_m / (sqrt(next_v) + e) with the OLD p in the decay term, which is what decoupled decay without bias correction computes:
    the two agree up to rounding (1e-3 of the bound asked here, two float64 runs)."""
    base, grads = C.draw(False)
    h = C.hyper("decoupled", bias_correction=False)
    mine = C.restatement(base, grads, h)
    b1, b2 = h["betas"]
    for i, b in enumerate(base):
        p, m, v = b.double().numpy().copy(), 0.0, 0.0
        for gs in grads:
            if gs[i] is None:
                continue
            g = gs[i].double().numpy()
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            p = p - h["lr"] * (m / (np.sqrt(v) + h["eps"]) + h["weight_decay"] * p)
        want = torch.from_numpy(p)
        assert ((mine["param"][i] - want).abs() <= 1e-3 * C.bound(want)).all(), i


def test_step_route():
    plain = [dict(C.hyper(), params=[]), dict(C.hyper(), params=[], lr=1e-3)]
    assert step_route(plain) == step_route(plain, "group") == "adam"                  # the calls this optimiser always made
    assert step_route(plain, "global") == "adamw"
    assert step_route([dict(C.hyper(), params=[], decoupled_weight_decay=True)]) == "adam"    # no decay to decouple
    for kw in (dict(decay="l2"), dict(decay="decoupled"), dict(amsgrad=True), dict(maximize=True), dict(bias_correction=False)):
        assert step_route(plain + [dict(C.hyper(**kw), params=[])]) == "adamw", kw
    with pytest.raises(ValueError, match="clip_scope"):
        step_route(plain, "tensor")
    p = [torch.zeros(3, requires_grad=True)]
    assert FusedAdam(p, lr=1e-3).route() == "adam" and FusedAdam(p, lr=1e-3, capturable=True, max_grad_norm=1.0).route() == "adam"
    assert FusedAdam(p, lr=1e-3, weight_decay=0.1).route() == "adamw"
    assert FusedAdam(p, lr=1e-3, capturable=True, clip_scope="global").route() == "adamw"
    # opt-in at construction: an optimiser built as plain Adam is not the extended one, whatever is set on it later
    assert not FusedAdam(p, lr=1e-3).extended and not FusedAdam(p, lr=1e-3, capturable=True, max_grad_norm=1.0).extended
    for kw in (dict(weight_decay=0.1), dict(decoupled_weight_decay=True), dict(amsgrad=True), dict(maximize=True), dict(bias_correction=False),
               dict(capturable=True, clip_scope="global")):
        assert FusedAdam(p, lr=1e-3, **kw).extended, kw
    assert FusedAdam([{"params": p, "weight_decay": 0.1}], lr=1e-3).extended                     # asked for in a group of `params`
    opt = FusedAdam(p, lr=1e-3)
    opt.param_groups[0]["amsgrad"] = True
    assert opt.route() == "adamw" and not opt.extended
    p[0].grad = torch.zeros(3)
    with pytest.raises(RuntimeError, match="built as plain Adam"):        # raised before anything touches the (CPU) tensors
        opt.step()
    with pytest.raises(ValueError, match="capturable"):
        FusedAdam(p, lr=1e-3, clip_scope="global")
    with pytest.raises(ValueError, match="clip_scope"):
        FusedAdam(p, lr=1e-3, capturable=True, clip_scope="tensor")
    with pytest.raises(ValueError, match="hyper-parameters"):
        FusedAdam(p, lr=1e-3, weight_decay=-0.1)


def test_the_extensions_symbols_declared_recorded_exported():
    """include/gcgcn_optim.h (symbols gcopt_*) is held the way tests/test_abi_cpu.py holds include/gcgcn.h: the parsed table
    equals the hand-written tests/golden/abi_signatures_optim.json entry by entry, every declared symbol resolves in the library,
    and the library exports no gcopt_* symbol that the header does not declare.  The core table is not touched."""
    sig = _lib.OPTIM_SIGNATURES
    names = {ctypes.c_int: "c_int", ctypes.c_int64: "c_int64", ctypes.c_double: "c_double", ctypes.c_void_p: "c_void_p"}
    with open(os.path.join(GOLDEN, "abi_signatures_optim.json")) as f:
        recorded = json.load(f)
    assert list(sig) == list(recorded) == ["gcopt_adamw_ws_bytes", "gcopt_adamw_step", "gcopt_adamw_step_dev"]
    for name, (res, args) in sig.items():
        assert {"restype": names[res], "argtypes": [names[a] for a in args]} == recorded[name], name
    assert not set(sig) & set(_lib.SIGNATURES) and all(n.startswith("gcgcn_") for n in _lib.SIGNATURES)
    assert _lib.ABI_VERSION == 7 and _lib.lib().gcgcn_version() == 7
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in sig:
        assert hasattr(handle, name), f"{name} is declared in include/gcgcn_optim.h but missing from the library"
    if shutil.which("nm") is not None:
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if re.fullmatch(r"gcopt_\w+", line.split()[-1])} == set(sig)
    # the capturable form: the host form's arguments, then max_norm, ws, ws_bytes, grad_norm in front of the stream
    assert sig["gcopt_adamw_step_dev"][1][:5] == sig["gcopt_adamw_step"][1][:5]
    assert sig["gcopt_adamw_step_dev"][1][5:] == _lib.SIGNATURES["gcgcn_adam_step_dev"][1][7:]
    with pytest.raises(RuntimeError, match="not a declaration"):           # a gcgcn_* declaration does not belong in that header
        _lib._parse_header("int gcgcn_x(int n);", _lib._DECL_OPTIM)
    assert "bert_param_groups" in gcgcn_amd.__all__


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 0.8, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, **kw):
        self.data_word_vec = np.zeros((30, 100), np.float32)
        self.__dict__.update(kw)


def _tiny():
    return BertConfig(vocab_size=40, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128,
                      max_position_embeddings=16)


def test_bert_param_groups():
    for model in (BertModel(_tiny()), M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_impl="torch", bert_config=_tiny()))):
        next(model.parameters()).requires_grad_(False)                    # a frozen parameter is in neither group
        groups = gcgcn_amd.bert_param_groups(model, 0.01)
        assert [g["weight_decay"] for g in groups] == [0.01, 0.0] and all(set(g) == {"params", "weight_decay"} for g in groups)
        named = {n: p for n, p in model.named_parameters() if p.requires_grad}
        ids = [id(p) for g in groups for p in g["params"]]
        assert len(ids) == len(set(ids)) == len(named) and set(ids) == {id(p) for p in named.values()}
        rest = {id(p) for p in groups[1]["params"]}
        want = {id(p) for n, p in named.items() if n.endswith("bias") or n.endswith("LayerNorm.weight")}
        assert rest == want and len(want) >= 8
        names_rest = sorted(n for n, p in named.items() if id(p) in rest)
        assert any(n.endswith("attention.output.LayerNorm.weight") for n in names_rest)
        assert all(not n.endswith("dense.weight") for n in names_rest)
        only_bias = gcgcn_amd.bert_param_groups(model, 0.01, no_decay=("bias",))
        assert {id(p) for p in only_bias[1]["params"]} == {id(p) for n, p in named.items() if n.endswith("bias")}
        FusedAdam(groups, lr=1e-4, decoupled_weight_decay=True)           # the groups are what the optimiser takes


def _cpu_steps(opt, params, grads, steps):
    for s in steps:
        C.set_grads(params, grads[s])
        opt.step()


def test_checkpoints_carry_torchs_keys():
    """torch.optim.AdamW / Adam state -> FusedAdam and back, on CPU tensors (nothing is stepped by FusedAdam here): torch's group
    keys arrive under torch's names, amsgrad's state is ``max_exp_avg_sq``, and a checkpoint without it gets zeros."""
    base, grads = C.draw(True)
    pa = C.make_params(base)
    oa = torch.optim.AdamW(pa, lr=C.LR, weight_decay=C.WD, amsgrad=True, betas=C.AMS_BETAS, foreach=False)
    _cpu_steps(oa, pa, grads, (0, 1))
    pb = C.make_params(base)
    ob = FusedAdam(pb, lr=1.0, weight_decay=0.5)                          # built for decay: what the checkpoint says then holds
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    g = ob.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["decoupled_weight_decay"], g["amsgrad"], g["maximize"]) == (C.LR, C.WD, True, True, False)
    assert g["betas"] == C.AMS_BETAS and g["bias_correction"] is True and g["capturable"] is False and ob.route() == "adamw" and ob.extended
    for a, b in zip(pa, pb):
        assert set(ob.state[b]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
        assert torch.equal(ob.state[b]["max_exp_avg_sq"], oa.state[a]["max_exp_avg_sq"])
    ob._check_group(g)                                                    # foreach=False / fused=None / differentiable=False: fine
    for key in ("foreach", "fused", "differentiable"):
        with pytest.raises(RuntimeError, match=key):
            FusedAdam._check_group(dict(g, **{key: True}))
    # a checkpoint written without amsgrad, loaded into an amsgrad group of either optimiser's making
    pc = C.make_params(base)
    oc = torch.optim.Adam(pc, lr=C.LR, foreach=False)
    _cpu_steps(oc, pc, grads, (0, 1))
    sd = copy.deepcopy(oc.state_dict())
    sd["param_groups"][0]["amsgrad"] = True
    od = FusedAdam(C.make_params(base), lr=C.LR, amsgrad=True)
    od.load_state_dict(sd)
    for p in od.param_groups[0]["params"]:
        st = od.state[p]
        assert torch.equal(st["max_exp_avg_sq"], torch.zeros_like(p)) and st["max_exp_avg_sq"].shape == st["exp_avg_sq"].shape
    # FusedAdam -> torch: its state_dict carries torch's keys, and torch's AdamW steps on from it
    out = od.state_dict()["param_groups"][0]
    for key in ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay", "amsgrad", "maximize", "capturable"):
        assert key in out, key
    pe = C.make_params(base)
    oe = torch.optim.Adam(pe, lr=C.LR, foreach=False)
    oe.load_state_dict(copy.deepcopy(od.state_dict()))
    assert oe.param_groups[0]["amsgrad"] is True and oe.param_groups[0]["decoupled_weight_decay"] is False
    _cpu_steps(oe, pe, grads, (2,))
    assert all(float(oe.state[p]["step"]) == (1.0 if i == C.LAGGING else 3.0) for i, p in enumerate(pe))     # it lags in steps 2 and 3


def test_a_group_without_rows_gets_no_record():
    """The image handed to gcopt_adamw_step / gcopt_adamw_step_dev: a parameter group that contributes no row (no parameters,
    or none with a gradient) is left out, the rows' group index counts the groups that are kept, and block_begin runs on.  The
    kernels read every record they are given -- the capturable form follows each record's lr pointer -- so a record that no row
    refers to must not be there."""
    from gcgcn_amd.optim import pack_adamw_image
    rec = lambda tag: [tag, tag + 1, tag + 2, tag + 3, 0xD0000 + tag, 2]
    row = lambda tag, n: (tag, tag + 1, tag + 2, tag + 3, 0, n, 0xA0000 + tag)
    image, n_rows, n_recs, blocks = pack_adamw_image([(rec(10), []), (rec(20), [row(100, 1025), row(200, 0)]), (rec(30), []),
                                                      (rec(40), [row(300, 7)]), (rec(50), [])])
    assert (n_rows, n_recs, blocks) == (3, 2, 3) and image.dtype == np.int64 and image.shape == (3 * 9 + 2 * 6,)
    rows, recs = image[:27].reshape(3, 9), image[27:].reshape(2, 6)
    assert rows[:, 0].tolist() == [100, 200, 300] and rows[:, 5].tolist() == [1025, 0, 7]
    assert rows[:, 6].tolist() == [0, 2, 2]                   # block_begin: 1025 elements own two workgroups, the empty tensor none
    assert rows[:, 8].tolist() == [0, 0, 1]                   # the group index counts the kept groups
    assert rows[:, 7].tolist() == [0xA0000 + 100, 0xA0000 + 200, 0xA0000 + 300]
    assert recs[:, 0].tolist() == [20, 40] and recs[:, 4].tolist() == [0xD0000 + 20, 0xD0000 + 40]      # only the kept groups' lr words
    assert all(int(r[8]) < n_recs for r in rows)
    empty = pack_adamw_image([(rec(10), []), (rec(20), [])])
    assert empty[1:] == (0, 0, 0) and empty[0].size == 0


def test_bert_param_groups_returns_no_empty_group():
    model = BertModel(_tiny())
    for name, p in model.named_parameters():                  # only biases and LayerNorm train
        p.requires_grad_(name.endswith(("bias", "LayerNorm.weight")))
    groups = gcgcn_amd.bert_param_groups(model, 0.01)
    assert len(groups) == 1 and groups[0]["weight_decay"] == 0.0 and len(groups[0]["params"]) == 13
    for p in model.parameters():
        p.requires_grad_(True)
    everything = gcgcn_amd.bert_param_groups(model, 0.01, no_decay=())
    assert len(everything) == 1 and everything[0]["weight_decay"] == 0.01 and len(everything[0]["params"]) == 23


def test_refusals_at_step():
    """What stays unsupported raises from step() before any tensor is touched (CPU tensors here): default-form and capturable
    groups mixed under clip_scope="global", unequal max_grad_norm under it, max_grad_norm in a default-form group; and
    add_param_group with a decayed group makes a plain optimiser the extended one, like the constructor."""
    a, b = torch.zeros(3, requires_grad=True), torch.zeros(4, requires_grad=True)
    a.grad, b.grad = torch.zeros(3), torch.zeros(4)
    opt = FusedAdam([{"params": [a]}, {"params": [b]}], lr=1e-3, weight_decay=0.1, capturable=True, max_grad_norm=1.0, clip_scope="global")
    opt.param_groups[1]["capturable"] = False
    opt.param_groups[1]["max_grad_norm"] = None
    with pytest.raises(RuntimeError, match="capturable=True in every parameter group"):
        opt.step()
    opt.param_groups[1]["capturable"] = True
    opt.param_groups[1]["max_grad_norm"] = 2.0
    with pytest.raises(RuntimeError, match="max_grad_norm must be the same"):
        opt.step()
    host = FusedAdam([a], lr=1e-3, weight_decay=0.1)
    host.param_groups[0]["max_grad_norm"] = 1.0
    with pytest.raises(RuntimeError, match="max_grad_norm needs capturable"):
        host.step()
    plain = FusedAdam([a], lr=1e-3)
    assert not plain.extended
    plain.add_param_group({"params": [b]})
    assert not plain.extended and plain.route() == "adam"
    grown = FusedAdam([a], lr=1e-3)
    grown.add_param_group({"params": [b], "weight_decay": 0.1})
    assert grown.extended and grown.route() == "adamw"


def test_parser_names_the_header_it_reads():
    with pytest.raises(RuntimeError, match=r"gcopt_x.*size_t.*include/gcgcn_optim\.h"):
        _lib._parse_header("int gcopt_x(size_t n);", _lib._DECL_OPTIM, "include/gcgcn_optim.h")
    with pytest.raises(RuntimeError, match=r"include/gcgcn_optim\.h: not a declaration"):
        _lib._parse_header("int other(int n);", _lib._DECL_OPTIM, "include/gcgcn_optim.h")
