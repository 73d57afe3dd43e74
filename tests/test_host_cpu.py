"""CPU-side tests (no GPU; the library's symbols against include/gcgcn.h: tests/test_abi_cpu.py): the option names,
parameter layouts agree between Python and the library, reference checkpoints round-trip through the
flat parameter buffers, and the product path refuses CPU tensors (no fallback)."""
import os
import re

import pytest
import torch

from conftest import ROOT, golden_files, load_golden
import gcgcn_amd
from gcgcn_amd import _lib, params as P


# gcgcn_set_option's names (api.hip g_opts) with their defaults, and names of switches that are constants now
OPTION_DEFAULTS = {"head_v1": -1, "head_bil3": 1, "head_bil3_bwd": 1, "head_dw3": 1, "head_compact": 1, "chain_t": 1,
                   "chain_big": 0, "split_widen": 1, "chain": 1, "mha_core": 1, "group_dump": 0}
RETIRED_OPTIONS = ["chain_fuse", "chain_carry", "att_in_chain", "maggc_fuse", "mha_ride", "gat_ride", "carry_spread",
                   "carry_cohort", "carry_spread_min", "chain_spread", "chain_cohort", "chain_spread_min", "fold_slices",
                   "head_sum_fold", "chain_s", "chain_t_wide_full"]


def test_set_option_knows_exactly_the_kept_options():
    """Every kept option is accepted (set to its default: the process is left as it was found), every retired one is refused,
    and every option a test or tool sets by a literal name is a kept one."""
    for name, dflt in OPTION_DEFAULTS.items():
        _lib.call("gcgcn_set_option", name.encode(), dflt)
    for name in RETIRED_OPTIONS:
        with pytest.raises(RuntimeError, match="unknown option"):
            _lib.call("gcgcn_set_option", name.encode(), 0)
    used = set()
    for d in ("tests", "tools"):
        for f in sorted(os.listdir(os.path.join(ROOT, d))):
            if f.endswith(".py"):
                used |= set(re.findall(r'gcgcn_set_option", b"(\w+)"', open(os.path.join(ROOT, d, f)).read()))
    used.discard("bogus")                        # (test_hip_parity's deliberately unknown name)
    assert used and used <= set(OPTION_DEFAULTS), used - set(OPTION_DEFAULTS)


@pytest.mark.parametrize("D,L,H", [(8, 2, 2), (128, 2, 8), (768, 4, 4), (512, 2, 8), (12, 4, 4)])
def test_layouts_match_library(D, L, H):
    assert P.gat_layout(D) == _lib.layout("gat", D, D)
    assert P.gat_layout(D, 2 * D + 3) == _lib.layout("gat", D, 2 * D + 3)          # att_input_dim != hidden_dim
    assert P.mha_layout(D) == _lib.layout("mha", D)
    assert P.gcn_layout(D, L, H) == _lib.layout("gcn", D, L, H)
    assert P.producer_layout(D, 20) == _lib.layout("producer", D, 20)                 # f1: edge-feature producer
    assert P.head_layout(D, L + 1, 20, 12, 97) == _lib.layout("head", D, L + 1, 20, 12, 97)   # f3: classifier head


def test_layout_errors_are_reported_not_fatal():
    with pytest.raises(RuntimeError, match="not divisible"):
        _lib.layout("gcn", 10, 3, 2)


@pytest.mark.parametrize("path", golden_files("stack"))
def test_reference_checkpoint_roundtrip(path):
    g = load_golden(path)
    m = g["meta"]
    hops = gcgcn_amd.GraphHops(m["d"], m["l"], m["h"])
    res = hops.load_state_dict(g["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = hops.state_dict()
    assert list(out.keys()) == list(g["sd"].keys())          # same keys, same order as the reference
    for k, v in g["sd"].items():
        assert out[k].shape == v.shape and torch.equal(out[k], v), k
    # parameter count equals the reference's (linears_k included)
    assert sum(p.numel() for p in hops.parameters()) == sum(v.numel() for v in g["sd"].values())


def test_strict_load_reports_missing_and_unexpected():
    hops = gcgcn_amd.GraphHops(8, 2, 2)
    sd = hops.state_dict()
    sd.pop("graphcnn.1.linear_layer.bias")
    sd["graphcnn.1.bogus"] = torch.zeros(1)
    with pytest.raises(RuntimeError) as ei:
        hops.load_state_dict(sd, strict=True)
    assert "graphcnn.1.linear_layer.bias" in str(ei.value) and "graphcnn.1.bogus" in str(ei.value)
    bad = hops.state_dict()
    bad["graphcnn.0.linear_layer.weight"] = torch.zeros(3, 3)
    with pytest.raises(RuntimeError, match="size mismatch"):
        hops.load_state_dict(bad)


def test_partial_checkpoint_loads_what_matches():
    """strict=False with some keys of a block missing: nn.Module semantics (which the reference follows) load the keys
    that are present and report the others."""
    torch.manual_seed(1)
    hops = gcgcn_amd.GraphHops(8, 2, 2)
    before = {k: v.clone() for k, v in hops.state_dict().items()}
    sd = {"graphcnn.1.graphconv.3.weights_node": torch.full((12, 4), 0.5),
          "get_weighted_adj_matrix.wt.bias": torch.tensor([7.0])}
    res = hops.load_state_dict(sd, strict=False)
    after = hops.state_dict()
    assert "graphcnn.1.linear_layer.bias" in res.missing_keys and not res.unexpected_keys
    for k in before:
        want = sd.get(k, before[k])
        assert torch.equal(after[k], want), k


def test_gat_rectangular_projection_state_dict():
    """GATAttention(att_input_dim, hidden_dim) with att_input_dim != hidden_dim: the reference's shapes (glove:148-151)."""
    m = gcgcn_amd.GATAttention(12, 20)
    sd = m.state_dict()
    assert sd["linear_node_h.weight"].shape == (20, 12) and sd["linear_edge_r.bias"].shape == (20,)
    assert sd["wt.weight"].shape == (1, 60)
    ref = torch.nn.Linear(12, 20)
    sd["linear_node_t.weight"] = ref.weight.detach().clone()
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.state_dict()["linear_node_t.weight"], ref.weight.detach())


def test_constructor_contract():
    with pytest.raises(AssertionError):
        gcgcn_amd.MultiHeadAttention(3, 8)                   # glove:125
    with pytest.raises(ValueError):
        gcgcn_amd.GraphConvolution(3, 8, 8)                  # D % L
    m = gcgcn_amd.MultiGraphConvolution(2, 4, 16, 16)
    # bias=True is accepted and ignored like the reference's blocks (glove:53/60, 83/94): same keys, no bias parameter
    assert list(gcgcn_amd.GraphConvolution(2, 16, 16, bias=True).state_dict()) == list(gcgcn_amd.GraphConvolution(2, 16, 16).state_dict())
    assert list(gcgcn_amd.MultiGraphConvolution(2, 4, 16, 16, bias=True).state_dict()) == list(m.state_dict())
    assert m.flat.numel() == sum(math_prod(s) for s in P.gcn_shapes(16, 2, 4).values())


def math_prod(s):
    n = 1
    for v in s:
        n *= v
    return n


def test_init_matches_reference_initialisers():
    """xavier-uniform bounds for weights_*, Linear default bounds elsewhere (glove:32-34)."""
    torch.manual_seed(0)
    D, L, H = 64, 2, 4
    t = gcgcn_amd.MultiGraphConvolution(L, H, D, D).named_tensors()
    gh = D // L
    we = t["graphconv.1.weights_edge"]
    assert we.abs().max() <= (6.0 / (D + gh)) ** 0.5 + 1e-6 and we.std() > 0.5 * (2.0 / (D + gh)) ** 0.5
    wn = t["graphconv.1.weights_node"]
    assert wn.shape == (D + gh, gh) and wn.abs().max() <= (6.0 / (D + 2 * gh)) ** 0.5 + 1e-6
    assert t["linear_layer.weight"].abs().max() <= 1.0 / (H * D) ** 0.5 + 1e-6


def test_no_cpu_fallback():
    hops = gcgcn_amd.GraphHops(8, 2, 2).eval()
    x, e = torch.zeros(3, 8), torch.zeros(3, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hops(x, [e, e])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.GATAttention(8, 8)(x, e)


def test_product_never_imports_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "gcgcn_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "oracle" not in src.replace("CPU oracle replay", ""), f"{f} mentions the oracle"


def test_bench_self_launches_its_ranks():
    """``python bench.py --gpus 2`` without a torch.distributed environment starts the two ranks itself (the driver may invoke
    the scaling runs the way it invokes the 1-GPU run).  On a box without GPUs the failure must come from the CHILDREN
    ("needs an MI355X"), not from a launcher hint, and the parent exits non-zero with their status."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"],
                       capture_output=True, text=True, env=env, timeout=300)
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the children would run the benchmark")
    assert r.returncode != 0
    assert "starting 2 ranks" in r.stderr
    assert "needs an MI355X" in r.stderr and "launch with" not in r.stderr
    assert r.stdout.strip() == ""                         # no JSON line from a failed run


def test_deferral_is_switched_off_under_ddp():
    """A forward that runs inside torch DistributedDataParallel's forward is recognised (its AccumulateGrad hooks need the
    gradient during backward, which a parked gradient does not give them): functional._under_ddp() is what the blocks ask."""
    import warnings
    import torch.distributed as dist
    from gcgcn_amd import functional as F_
    from torch.nn.parallel import DistributedDataParallel as DDP
    seen = []

    class Probe(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(2))

        def forward(self, x):
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                seen.append((F_._under_ddp(), [str(w.message) for w in rec]))
            return (x * self.w).sum()

    assert F_._under_ddp() is False
    m = Probe()
    m(torch.ones(2))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        os.environ["MASTER_PORT"] = str(so.getsockname()[1])
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        F_._warned_ddp[0] = False
        DDP(m)(torch.ones(2)).backward()
    finally:
        dist.destroy_process_group()
    assert seen[0][0] is False and seen[1][0] is True
    assert any("DistributedDataParallel" in w for w in seen[1][1])
    assert F_._under_ddp() is False
    # a torch build without the private marker: the test fails CLOSED (no parking) once several ranks exist, and stays off alone
    saved = DDP._active_ddp_module
    try:
        del DDP._active_ddp_module
        assert F_._under_ddp() is False                      # no process group: nothing to protect
        real = (dist.is_initialized, dist.get_world_size)
        dist.is_initialized, dist.get_world_size = (lambda: True), (lambda *a, **k: 2)
        try:
            assert F_._under_ddp() is True
        finally:
            dist.is_initialized, dist.get_world_size = real
    finally:
        DDP._active_ddp_module = saved


def test_tail_keys_as_root_and_as_submodule():
    """GraphModelTail's state_dict carries the MODEL's key names (word_attention.{i}.*, dense_layer.*, ...) both as the root
    module and nested in a parent (the documented integration: embeddings / encoder live in the parent), load_state_dict
    accepts them in both positions, strict, and the dict's _metadata survives."""
    torch.manual_seed(0)
    tail = gcgcn_amd.GraphModelTail(hidden_size=16, layer_num=2, head_num=2, dis_size=4, entity_type_size=4, relation_num=5)

    class Parent(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.dis_embed = torch.nn.Embedding(21, 4)
            self.tail = gcgcn_amd.GraphModelTail(hidden_size=16, layer_num=2, head_num=2, dis_size=4, entity_type_size=4, relation_num=5)

    root_sd = tail.state_dict()
    assert hasattr(root_sd, "_metadata")
    assert "word_attention.1.attention_sent.weight" in root_sd and "dense_layer.weight" in root_sd
    assert not any(k.startswith(("producers.", "head.")) for k in root_sd)
    par = Parent()
    psd = par.state_dict()
    assert "tail.word_attention.0.attention_all.bias" in psd and "tail.bili_layer_01.weight" in psd and "dis_embed.weight" in psd
    assert not any(".producers." in k or ".head." in k for k in psd)
    assert [k[len("tail."):] for k in psd if k.startswith("tail.")] == list(root_sd)          # same keys, same order
    # round trips: root -> nested, nested -> root, strict
    src = {("tail." + k): v + 1.0 for k, v in root_sd.items()}
    src["dis_embed.weight"] = psd["dis_embed.weight"]
    assert par.load_state_dict(src, strict=True).missing_keys == []
    for k, v in par.tail.state_dict().items():
        torch.testing.assert_close(v, root_sd[k] + 1.0)
    tail.load_state_dict({k[len("tail."):]: v for k, v in par.state_dict().items() if k.startswith("tail.")}, strict=True)
    for k, v in tail.state_dict().items():
        torch.testing.assert_close(v, root_sd[k] + 1.0)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        tail.load_state_dict({**root_sd, "word_attention.7.attention_sent.weight": torch.zeros(1)}, strict=True)


@pytest.mark.parametrize("tiles,others,cohort,pct", [(0, 100, 256, 90), (357, 2176, 256, 0), (1536, 8192, 256, 90), (2208, 8192, 256, 90),
                                                      (2376, 2112, 256, 90), (336, 8192, 128, 85), (224, 2048, 128, 85), (7, 3, 8, 100),
                                                      (1000, 10, 256, 90), (513, 4099, 64, 50), (1, 1, 1, 100)])
def test_tile_passengers_and_rows_each_get_exactly_one_workgroup(tiles, others, cohort, pct):
    """csrc/common.hpp Spread / spread_pick (the function the carrying kernels call, here run on the host): over the
    tiles + others workgroup indices of a launch every tile ordinal and every row ordinal appears exactly once, tiles come in
    cohorts of `cohort` consecutive workgroups, a cohort's first workgroup index is a multiple of 8 whenever the cohort is
    (xcd_remap's low bits), and pct = 0 puts every tile in front."""
    import ctypes
    import numpy as np
    from gcgcn_amd import _lib
    n = tiles + others
    kind = np.full(n, -1, np.int32)
    ordinal = np.full(n, -1, np.int32)
    _lib.call("gcgcn_debug_spread", tiles, others, cohort, pct, kind.ctypes.data_as(ctypes.c_void_p), ordinal.ctypes.data_as(ctypes.c_void_p))
    t_idx = np.flatnonzero(kind == 1)
    r_idx = np.flatnonzero(kind == 0)
    assert len(t_idx) == tiles and len(r_idx) == others
    assert np.array_equal(ordinal[t_idx], np.arange(tiles))            # in order, each exactly once
    assert np.array_equal(ordinal[r_idx], np.arange(others))
    if pct == 0 and tiles:
        assert t_idx[-1] == tiles - 1
    for c0 in range(0, tiles, cohort):                                 # a cohort is one run of consecutive workgroups
        run = t_idx[c0:c0 + cohort]
        assert np.array_equal(run, np.arange(run[0], run[0] + len(run)))
        if cohort % 8 == 0:
            assert run[0] % 8 == 0


# (label, B, N, D, L, H): the bench shapes, the golden-fixture shapes, and graph sizes either side of the kernels' limits
CHAIN_PLAN_SHAPES = [("c1", 8, 16, 128, 2, 8), ("c2", 32, 64, 256, 2, 8), ("c2/H1", 32, 64, 256, 2, 1), ("c3", 32, 64, 768, 4, 4),
                     ("c5", 32, 256, 512, 2, 8), ("g7", 2, 7, 12, 4, 4), ("g16a", 2, 16, 64, 4, 4), ("g16b", 2, 16, 128, 2, 8),
                     ("g5", 2, 5, 8, 2, 2), ("n48", 32, 48, 256, 2, 8), ("n128", 32, 128, 256, 2, 8)]
# (label, option to set or None, value, misalign bits, scratch given)
CHAIN_PLAN_VARIANTS = [("default", None, 0, 0, 1), ("misalign=tensors", None, 0, 1, 1), ("misalign=dout", None, 0, 2, 1),
                       ("misalign=ride", None, 0, 4, 1), ("misalign=flat", None, 0, 8, 1), ("misalign=all", None, 0, 15, 1),
                       ("no scratch", None, 0, 0, 0), ("chain=0", "chain", 0, 0, 1), ("chain_big=1", "chain_big", 1, 0, 1),
                       ("chain_t=0", "chain_t", 0, 0, 1), ("chain_t=1", "chain_t", 1, 0, 1), ("chain_t=2", "chain_t", 2, 0, 1)]


def chain_plan_table(plan, set_option, hook_allowed):
    """One line per (shape, variant): the plan of forward (dense / ragged) x (no ride / ride) x (no hook / hook), then of backward
    (dense / ragged) x (no ride / ride), each as the kind's letter (n one launch per product, g generic, s, t) followed by the
    letters of the bits that are set: a aligned, F full, u fuse, x attention, r ride; '-' where the attention hook may not be
    given.  plan(bwd, B, N, D, L, H, ragged, ride, hook, scratch, misalign) -> six ints."""
    lines = []
    for label, B, N, D, L, H in CHAIN_PLAN_SHAPES:
        for vlabel, opt, value, misalign, scratch in CHAIN_PLAN_VARIANTS:
            codes = []
            try:
                if opt:
                    set_option(opt, value)
                for bwd in (0, 1):
                    for ragged in (0, 1):
                        for ride in (0, 1):
                            for hook in ((0,) if bwd else (0, 1)):
                                if hook and not hook_allowed(N, D, H):
                                    codes.append("-")
                                    continue
                                out = plan(bwd, B, N, D, L, H, ragged, ride, hook, scratch, misalign)
                                codes.append("ngst"[out[0]] + "".join(c for c, bit in zip("aFuxr", out[1:]) if bit))
            finally:
                if opt:
                    set_option(opt, OPTION_DEFAULTS[opt])
            lines.append(f"{label:6s}{vlabel:17s}: " + " ".join(codes))
    return lines


# Recorded from the PARENT of the commit that introduced chain_plan_fwd / _bwd, not from the code under test: in a scratch copy of
# the parent a throw-away function evaluated the parent's own predicates (use_chain_for, chain_can_carry, chain_bwd_fusable + the
# alignment tests of dXres / dout / dout_m, chain_fwd_computes_attention, then chain_aligned, chain_small_ok, chain_t_ok,
# chain_s_preferred, chain_t_full and the FUSE choice of chain_t_run_bwd) in the order gcgcn_gcn_fwd / _bwd and gcn_chain_fwd /
# _bwd evaluated them, on the operand addresses gcgcn_debug_chain_plan makes up, and chain_plan_table printed this.
CHAIN_PLAN_EXPECTED = """
c1    default          : t tx tr txr t tx tr txr tu tur tu tur
c1    misalign=tensors : g g gr gr g g gr gr g gr g gr
c1    misalign=dout    : t tx tr txr t tx tr txr t tr t tr
c1    misalign=ride    : t tx t tx t tx t tx tu tu tu tu
c1    misalign=flat    : g g gr gr g g gr gr g gr g gr
c1    misalign=all     : g g g g g g g g g g g g
c1    no scratch       : t tx tr txr t tx tr txr t tr t tr
c1    chain=0          : n n n n n n n n n n n n
c1    chain_big=1      : t tx tr txr t tx tr txr tu tur tu tur
c1    chain_t=0        : g g gr gr g g gr gr g gr g gr
c1    chain_t=1        : t tx tr txr t tx tr txr tu tur tu tur
c1    chain_t=2        : t tx tr txr t tx tr txr tu tur tu tur
c2    default          : s sx sr sxr t tx tr txr su sur tu tur
c2    misalign=tensors : g g gr gr g g gr gr g gr g gr
c2    misalign=dout    : s sx sr sxr t tx tr txr s sr t tr
c2    misalign=ride    : s sx s sx t tx t tx su su tu tu
c2    misalign=flat    : g g gr gr g g gr gr g gr g gr
c2    misalign=all     : g g g g g g g g g g g g
c2    no scratch       : s sx sr sxr t tx tr txr s sr t tr
c2    chain=0          : n n n n n n n n n n n n
c2    chain_big=1      : s sx sr sxr t tx tr txr su sur tu tur
c2    chain_t=0        : s sx sr sxr s sx sr sxr su sur su sur
c2    chain_t=1        : s sx sr sxr t tx tr txr su sur tu tur
c2    chain_t=2        : tF tFx tFr tFxr t tx tr txr tFu tFur tu tur
c2/H1 default          : s s sr sr t tx tr txr su sur tu tur
c2/H1 misalign=tensors : g g gr gr g g gr gr g gr g gr
c2/H1 misalign=dout    : s s sr sr t tx tr txr s sr t tr
c2/H1 misalign=ride    : s s s s t tx t tx su su tu tu
c2/H1 misalign=flat    : g g gr gr g g gr gr g gr g gr
c2/H1 misalign=all     : g g g g g g g g g g g g
c2/H1 no scratch       : s s sr sr t tx tr txr s sr t tr
c2/H1 chain=0          : n n n n n n n n n n n n
c2/H1 chain_big=1      : s s sr sr t tx tr txr su sur tu tur
c2/H1 chain_t=0        : s s sr sr s s sr sr su sur su sur
c2/H1 chain_t=1        : s s sr sr t tx tr txr su sur tu tur
c2/H1 chain_t=2        : tF tFx tFr tFxr t tx tr txr tFu tFur tu tur
c3    default          : tF tFx tFr tFxr t tx tr txr tF tFr t tr
c3    misalign=tensors : g g gr gr g g gr gr g gr g gr
c3    misalign=dout    : tF tFx tFr tFxr t tx tr txr tF tFr t tr
c3    misalign=ride    : tF tFx tF tFx t tx t tx tF tF t t
c3    misalign=flat    : g g gr gr g g gr gr g gr g gr
c3    misalign=all     : g g g g g g g g g g g g
c3    no scratch       : tF tFx tFr tFxr t tx tr txr tF tFr t tr
c3    chain=0          : n n n n n n n n n n n n
c3    chain_big=1      : tF tFx tFr tFxr t tx tr txr tF tFr t tr
c3    chain_t=0        : ga ga gar gar ga ga gar gar ga gar ga gar
c3    chain_t=1        : tF tFx tFr tFxr t tx tr txr tF tFr t tr
c3    chain_t=2        : tF tFx tFr tFxr t tx tr txr tF tFr t tr
c5    default          : n - gar - n - gar - n n n n
c5    misalign=tensors : n - gr - n - gr - n n n n
c5    misalign=dout    : n - gar - n - gar - n n n n
c5    misalign=ride    : n - n - n - n - n n n n
c5    misalign=flat    : n - gr - n - gr - n n n n
c5    misalign=all     : n - n - n - n - n n n n
c5    no scratch       : n - gar - n - gar - n n n n
c5    chain=0          : n - n - n - n - n n n n
c5    chain_big=1      : ga - gar - ga - gar - ga gar ga gar
c5    chain_t=0        : n - gar - n - gar - n n n n
c5    chain_t=1        : n - gar - n - gar - n n n n
c5    chain_t=2        : n - gar - n - gar - n n n n
g7    default          : g - gr - g - gr - g gr g gr
g7    misalign=tensors : g - gr - g - gr - g gr g gr
g7    misalign=dout    : g - gr - g - gr - g gr g gr
g7    misalign=ride    : g - g - g - g - g g g g
g7    misalign=flat    : g - gr - g - gr - g gr g gr
g7    misalign=all     : g - g - g - g - g g g g
g7    no scratch       : g - gr - g - gr - g gr g gr
g7    chain=0          : n - n - n - n - n n n n
g7    chain_big=1      : g - gr - g - gr - g gr g gr
g7    chain_t=0        : g - gr - g - gr - g gr g gr
g7    chain_t=1        : g - gr - g - gr - g gr g gr
g7    chain_t=2        : g - gr - g - gr - g gr g gr
g16a  default          : g g gr gr g g gr gr g gr g gr
g16a  misalign=tensors : g g gr gr g g gr gr g gr g gr
g16a  misalign=dout    : g g gr gr g g gr gr g gr g gr
g16a  misalign=ride    : g g g g g g g g g g g g
g16a  misalign=flat    : g g gr gr g g gr gr g gr g gr
g16a  misalign=all     : g g g g g g g g g g g g
g16a  no scratch       : g g gr gr g g gr gr g gr g gr
g16a  chain=0          : n n n n n n n n n n n n
g16a  chain_big=1      : g g gr gr g g gr gr g gr g gr
g16a  chain_t=0        : g g gr gr g g gr gr g gr g gr
g16a  chain_t=1        : g g gr gr g g gr gr g gr g gr
g16a  chain_t=2        : g g gr gr g g gr gr g gr g gr
g16b  default          : t tx tr txr t tx tr txr tu tur tu tur
g16b  misalign=tensors : g g gr gr g g gr gr g gr g gr
g16b  misalign=dout    : t tx tr txr t tx tr txr t tr t tr
g16b  misalign=ride    : t tx t tx t tx t tx tu tu tu tu
g16b  misalign=flat    : g g gr gr g g gr gr g gr g gr
g16b  misalign=all     : g g g g g g g g g g g g
g16b  no scratch       : t tx tr txr t tx tr txr t tr t tr
g16b  chain=0          : n n n n n n n n n n n n
g16b  chain_big=1      : t tx tr txr t tx tr txr tu tur tu tur
g16b  chain_t=0        : g g gr gr g g gr gr g gr g gr
g16b  chain_t=1        : t tx tr txr t tx tr txr tu tur tu tur
g16b  chain_t=2        : t tx tr txr t tx tr txr tu tur tu tur
g5    default          : g g gr gr g g gr gr g gr g gr
g5    misalign=tensors : g g gr gr g g gr gr g gr g gr
g5    misalign=dout    : g g gr gr g g gr gr g gr g gr
g5    misalign=ride    : g g g g g g g g g g g g
g5    misalign=flat    : g g gr gr g g gr gr g gr g gr
g5    misalign=all     : g g g g g g g g g g g g
g5    no scratch       : g g gr gr g g gr gr g gr g gr
g5    chain=0          : n n n n n n n n n n n n
g5    chain_big=1      : g g gr gr g g gr gr g gr g gr
g5    chain_t=0        : g g gr gr g g gr gr g gr g gr
g5    chain_t=1        : g g gr gr g g gr gr g gr g gr
g5    chain_t=2        : g g gr gr g g gr gr g gr g gr
n48   default          : t tx tr txr t tx tr txr tu tur tu tur
n48   misalign=tensors : g g gr gr g g gr gr g gr g gr
n48   misalign=dout    : t tx tr txr t tx tr txr t tr t tr
n48   misalign=ride    : t tx t tx t tx t tx tu tu tu tu
n48   misalign=flat    : g g gr gr g g gr gr g gr g gr
n48   misalign=all     : g g g g g g g g g g g g
n48   no scratch       : t tx tr txr t tx tr txr t tr t tr
n48   chain=0          : n n n n n n n n n n n n
n48   chain_big=1      : t tx tr txr t tx tr txr tu tur tu tur
n48   chain_t=0        : g g gr gr g g gr gr g gr g gr
n48   chain_t=1        : t tx tr txr t tx tr txr tu tur tu tur
n48   chain_t=2        : t tx tr txr t tx tr txr tu tur tu tur
n128  default          : n - gar - n - gar - n n n n
n128  misalign=tensors : n - gr - n - gr - n n n n
n128  misalign=dout    : n - gar - n - gar - n n n n
n128  misalign=ride    : n - n - n - n - n n n n
n128  misalign=flat    : n - gr - n - gr - n n n n
n128  misalign=all     : n - n - n - n - n n n n
n128  no scratch       : n - gar - n - gar - n n n n
n128  chain=0          : n - n - n - n - n n n n
n128  chain_big=1      : ga - gar - ga - gar - ga gar ga gar
n128  chain_t=0        : n - gar - n - gar - n n n n
n128  chain_t=1        : n - gar - n - gar - n n n n
n128  chain_t=2        : n - gar - n - gar - n n n n
"""


def test_chain_plan_is_the_decision_the_scattered_predicates_made():
    """gcgcn_debug_chain_plan (the plan function gcgcn_gcn_fwd / _bwd call) gives, for every row, the kernel and the dependent
    bits the code before it chose.  No tolerance, no row left out."""
    import ctypes
    import numpy as np

    def plan(*args):
        out = np.full(6, -1, np.int32)
        _lib.call("gcgcn_debug_chain_plan", *args, out.ctypes.data_as(ctypes.c_void_p))
        return [int(v) for v in out]

    got = chain_plan_table(plan, lambda name, v: _lib.call("gcgcn_set_option", name.encode(), v),
                           lambda N, D, H: bool(_lib.lib().gcgcn_maggc_fusable(N, D, H)))
    want = CHAIN_PLAN_EXPECTED.strip("\n").split("\n")
    assert len(got) == len(want) == len(CHAIN_PLAN_SHAPES) * len(CHAIN_PLAN_VARIANTS)
    wrong = [f"want {w}\n got {g}" for g, w in zip(got, want) if g != w]
    assert not wrong, "\n".join(wrong)


# (B, N) of 1 000 pairs, and of 32 640 / 32 641: either side of the size rule (a 128-pair tile per compute unit: 256 tiles)
HEAD_PLAN_SHAPES = [(10, 10), (510, 8), (32641, 1)]
HEAD_PLAN_R = [5, 64, 65, 97, 98, 128]
HEAD_PLAN_OPTIONS = ["head_v1", "head_bil3", "head_bil3_bwd", "head_dw3", "head_compact"]
# a plan as four characters: compacted rows (c) or not (.); the forward pass, then the d eh / d et passes: g first-generation GEMM,
# s 64-pair tiles, b 128-pair tiles, B 128-pair tiles in both launch shapes (the device-side pair count selects one); d W_b: g GEMM,
# r all rows per workgroup
HEAD_PLAN_LEGEND = {"a": ".bbg", "b": ".bbr", "c": ".bgg", "d": ".bsg", "e": ".bsr", "f": ".ggg", "g": ".sbg", "h": ".sbr", "i": ".ssg",
                    "j": ".ssr", "k": "cBBr", "l": "cBsr", "m": "csBr", "n": "cssr"}


def head_plan_table(plan, set_option):
    """One line per setting of the five head options (head_v1 in -1, 0, 1; the others 0, 1): a group per shape, in it one plan per
    R and dense / ragged (ragged varying fastest), as the four characters HEAD_PLAN_LEGEND explains.
    plan(B, N, R, ragged) -> six ints."""
    import itertools
    lines = []
    try:
        for values in itertools.product((-1, 0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
            for name, v in zip(HEAD_PLAN_OPTIONS, values):
                set_option(name, v)
            groups = []
            for B, N in HEAD_PLAN_SHAPES:
                codes = []
                for R in HEAD_PLAN_R:
                    for ragged in (0, 1):
                        compact, fwd, bwd_e, dw, by_f, by_b = plan(B, N, R, ragged)
                        codes.append(".c"[compact] + ("GSB" if by_f else "gsb")[fwd] + ("GSB" if by_b else "gsb")[bwd_e] + "gr"[dw])
                groups.append(codes)
            lines.append((values, groups))
    finally:
        for name in HEAD_PLAN_OPTIONS:
            set_option(name, OPTION_DEFAULTS[name])
    return lines


# Recorded from the PARENT of the commit that introduced head_plan, not from the code under test: in a scratch copy of the parent a
# throw-away function evaluated the parent's own predicates (head_compacts, head_bil3_ok, head_v1, the tile choice and the
# both-shapes test of head_bil2, the head_dw3 condition) in the order head_fwd, head_bwd and head_bil2 evaluated them, and
# head_plan_table printed this with each distinct plan given a letter (HEAD_PLAN_LEGEND).  1 728 plans: a line per option setting
# (head_v1, head_bil3, head_bil3_bwd, head_dw3, head_compact), a group per shape (1 000, 32 640, 32 641 pairs).
HEAD_PLAN_EXPECTED = """
-1  0  0  0  0 : ffffffffffff ffffffffffff iiiiiiiiiiii
-1  0  0  0  1 : fffffnfnffff fffffnfnffff iiiiininiiii
-1  0  0  1  0 : ffffffffffff ffffffffffff iiiijjjjiiii
-1  0  0  1  1 : fffffnfnffff fffffnfnffff iiiijnjniiii
-1  0  1  0  0 : ffffffffffff ffffffffffff gggggggggggg
-1  0  1  0  1 : fffffmfmffff fffffmfmffff gggggmgmgggg
-1  0  1  1  0 : ffffffffffff ffffffffffff gggghhhhgggg
-1  0  1  1  1 : fffffmfmffff fffffmfmffff gggghmhmgggg
-1  1  0  0  0 : ffffccccffff ffffccccffff iiiiddddiiii
-1  1  0  0  1 : ffffclclffff ffffclclffff iiiidldliiii
-1  1  0  1  0 : ffffccccffff ffffccccffff iiiieeeeiiii
-1  1  0  1  1 : ffffclclffff ffffclclffff iiiieleliiii
-1  1  1  0  0 : ffffccccffff ffffccccffff ggggaaaagggg
-1  1  1  0  1 : ffffckckffff ffffckckffff ggggakakgggg
-1  1  1  1  0 : ffffccccffff ffffccccffff ggggbbbbgggg
-1  1  1  1  1 : ffffckckffff ffffckckffff ggggbkbkgggg
 0  0  0  0  0 : iiiiiiiiiiii iiiiiiiiiiii iiiiiiiiiiii
 0  0  0  0  1 : iiiiininiiii iiiiininiiii iiiiininiiii
 0  0  0  1  0 : iiiijjjjiiii iiiijjjjiiii iiiijjjjiiii
 0  0  0  1  1 : iiiijnjniiii iiiijnjniiii iiiijnjniiii
 0  0  1  0  0 : gggggggggggg gggggggggggg gggggggggggg
 0  0  1  0  1 : gggggmgmgggg gggggmgmgggg gggggmgmgggg
 0  0  1  1  0 : gggghhhhgggg gggghhhhgggg gggghhhhgggg
 0  0  1  1  1 : gggghmhmgggg gggghmhmgggg gggghmhmgggg
 0  1  0  0  0 : iiiiddddiiii iiiiddddiiii iiiiddddiiii
 0  1  0  0  1 : iiiidldliiii iiiidldliiii iiiidldliiii
 0  1  0  1  0 : iiiieeeeiiii iiiieeeeiiii iiiieeeeiiii
 0  1  0  1  1 : iiiieleliiii iiiieleliiii iiiieleliiii
 0  1  1  0  0 : ggggaaaagggg ggggaaaagggg ggggaaaagggg
 0  1  1  0  1 : ggggakakgggg ggggakakgggg ggggakakgggg
 0  1  1  1  0 : ggggbbbbgggg ggggbbbbgggg ggggbbbbgggg
 0  1  1  1  1 : ggggbkbkgggg ggggbkbkgggg ggggbkbkgggg
 1  0  0  0  0 : ffffffffffff ffffffffffff ffffffffffff
 1  0  0  0  1 : fffffnfnffff fffffnfnffff fffffnfnffff
 1  0  0  1  0 : ffffffffffff ffffffffffff ffffffffffff
 1  0  0  1  1 : fffffnfnffff fffffnfnffff fffffnfnffff
 1  0  1  0  0 : ffffffffffff ffffffffffff ffffffffffff
 1  0  1  0  1 : fffffmfmffff fffffmfmffff fffffmfmffff
 1  0  1  1  0 : ffffffffffff ffffffffffff ffffffffffff
 1  0  1  1  1 : fffffmfmffff fffffmfmffff fffffmfmffff
 1  1  0  0  0 : ffffccccffff ffffccccffff ffffccccffff
 1  1  0  0  1 : ffffclclffff ffffclclffff ffffclclffff
 1  1  0  1  0 : ffffccccffff ffffccccffff ffffccccffff
 1  1  0  1  1 : ffffclclffff ffffclclffff ffffclclffff
 1  1  1  0  0 : ffffccccffff ffffccccffff ffffccccffff
 1  1  1  0  1 : ffffckckffff ffffckckffff ffffckckffff
 1  1  1  1  0 : ffffccccffff ffffccccffff ffffccccffff
 1  1  1  1  1 : ffffckckffff ffffckckffff ffffckckffff
"""


def test_head_plan_is_the_decision_the_scattered_predicates_made():
    """gcgcn_debug_head_plan (the plan function gcgcn_head_fwd / _bwd call) gives, for every shape and every setting of the five head
    options, the kernels the code before it chose.  No tolerance, no row left out."""
    import ctypes
    import numpy as np

    def plan(*args):
        out = np.full(6, -1, np.int32)
        _lib.call("gcgcn_debug_head_plan", *args, out.ctypes.data_as(ctypes.c_void_p))
        return [int(v) for v in out]

    got = head_plan_table(plan, lambda name, v: _lib.call("gcgcn_set_option", name.encode(), v))
    want = HEAD_PLAN_EXPECTED.strip("\n").split("\n")
    assert len(got) == len(want) == 48
    rows, wrong = 0, []
    for (values, groups), line in zip(got, want):
        label, letters = line.split(" : ")
        assert [int(v) for v in label.split()] == list(values)
        for (B, N), codes, group in zip(HEAD_PLAN_SHAPES, groups, letters.split(" ")):
            assert len(codes) == len(group) == 2 * len(HEAD_PLAN_R)
            for k, (code, letter) in enumerate(zip(codes, group)):
                rows += 1
                if code != HEAD_PLAN_LEGEND[letter]:
                    wrong.append(f"options {values} B {B} N {N} R {HEAD_PLAN_R[k // 2]} ragged {k % 2}: want {HEAD_PLAN_LEGEND[letter]} got {code}")
    assert rows == 1728
    assert not wrong, "\n".join(wrong[:40])


# ---- the edge passes' plan ----------------------------------------------------------------------------------------------------
EDGE_PLAN_FIELDS = ["vec", "att", "route", "slices", "ngat", "lds", "lds_ok", "carry_ok", "RB", "grid", "col_base", "ncolwg", "sp_na",
                    "sp_cohort", "sp_stride", "scratch", "rowbuf_off"]
EDGE_PLAN_ARGS = ["pass", "compact", "B", "N", "D", "ragged", "att", "has_dE", "has_dEbar", "misalign", "parked_tiles", "any_rb", "col_C"]
# the constants the limits are computed from (not found by trial): EW / CW4 waves per workgroup, GT (gat_body.hpp), the 64 x 64 tile's
# LDS image lds_floats<1, 1, true, true>() with BK = 32 (gemm_body.hpp), the two LDS limits of edge.hip
EDGE_WAVES = 4
EDGE_GAT_DOC_LDS = 64 * 65 + 64
EDGE_TILE_LDS = ((2 * 32 * 65 + 3) & ~3) + 2 * 32 * 65
EDGE_LDS_MAX, EDGE_CMP_LDS_MAX = 160 * 1024 // 4, 64 * 1024 // 4   # floats
EDGE_CMP_MAX_D = 512


def edge_plan_sweep():
    """The argument rows (EDGE_PLAN_ARGS) of the plan table: every pass on dense and compact operands over the N and D steps, each
    misalignment bit alone and none, ragged / att / has_dE / has_dEbar on and off, the defer-queue summaries around the
    spread_min rule, and the sizes either side of each LDS threshold."""
    NS, DS, MIS = (1, 63, 64, 65, 100, 256), (1, 3, 4, 63, 64, 66, 252, 256, 260, 512, 516), (0, 1, 2, 4, 8, 16)
    B, rows = 3, []

    def row(ps, compact, N, D, B=B, ragged=0, att=1, has_dE=1, has_dEbar=1, mis=0, parked=0, any_rb=0, col_C=0):
        rows.append((ps, compact, B, N, D, ragged, att, has_dE, has_dEbar, mis, parked, any_rb, col_C))

    for N in NS:
        for D in DS:
            for mis in MIS:
                for att in (0, 1):
                    row(0, 0, N, D, att=att, mis=mis)                      # dense forward
                for has_dE in (0, 1):
                    row(1, 0, N, D, has_dE=has_dE, mis=mis)                # dense backward, nothing parked
                row(2, 0, N, D, att=0, mis=mis)                            # dense mean backward
            for ragged in (0, 1):
                for att in (0, 1):
                    row(0, 0, N, D, ragged=ragged, att=att, has_dE=0, has_dEbar=0)
                    if D <= EDGE_CMP_MAX_D:
                        row(0, 1, N, D, ragged=ragged, att=att)           # compact forward, backward (att 0: the mean alone)
                        row(1, 1, N, D, ragged=ragged, att=att)
                row(1, 0, N, D, ragged=ragged, has_dEbar=0, mis=8)         # an absent dEbar's alignment does not count
                row(1, 0, N, D, ragged=ragged, has_dE=0, mis=4)
                if D <= EDGE_CMP_MAX_D:
                    row(2, 1, N, D, ragged=ragged, att=0)
    # the queue summary: around spread_min = 1024, with and without row blocks and a column-sum second stage (256 columns per
    # workgroup), on shapes that may carry (vec 4) and that may not (D % 4 != 0, a misaligned E), with and without GAT passengers
    for N in (64, 65, 100):
        for D, mis in ((4, 0), (64, 0), (256, 0), (66, 0), (64, 1)):
            for parked in (0, 1, 1023, 1024, 5000):
                for any_rb in (0, 1):
                    for col_C in (0, 256, 257):
                        row(1, 0, N, D, mis=mis, parked=parked, any_rb=any_rb, col_C=col_C)
    # dense backward: a row's LDS (N rounded up to 4, + EW * D floats) crosses the GAT passenger's image, the tile's, the 160 KB limit
    for N in (64, 65, 256):
        N4 = (N + 3) & ~3
        for floats in (EDGE_GAT_DOC_LDS, EDGE_TILE_LDS, EDGE_LDS_MAX):
            d = (floats - N4) // EDGE_WAVES
            for D in (d - 4, d, d + 4):
                for parked in (0, 1024):
                    row(1, 0, N, D, B=1, parked=parked, col_C=256)
    # forward: the dense 160 KB limit and the compact 64 KB limit (EW * D + N floats with attention, EW * D without)
    for N in (64, 256):
        d = (EDGE_LDS_MAX - N) // EDGE_WAVES
        for D in (d - 4, d, d + 4, EDGE_LDS_MAX // EDGE_WAVES, EDGE_LDS_MAX // EDGE_WAVES + 4):
            for att in (0, 1):
                row(0, 0, N, D, B=1, att=att)
    for D in (EDGE_CMP_MAX_D - 4, EDGE_CMP_MAX_D):
        n = EDGE_CMP_LDS_MAX - EDGE_WAVES * D
        for N in (n - 1, n, n + 1):
            for att in (0, 1):
                row(0, 1, N, D, B=1, att=att)
                row(1, 1, N, D, B=1, att=att)
    return rows


def test_edge_plan_is_the_decision_the_scattered_expressions_made():
    """gcgcn_debug_edge_plan (the plan functions edge_fwd / edge_bwd / edge_bcast / cmp_fwd / cmp_bwd and the GATAttention entry
    points call) gives, for every row of edge_plan_sweep, the launch the code before it chose.  The expected table
    (tests/golden/edge_plan_parent.npz) was recorded from the PARENT of the commit that introduced EdgePlan, not from the code under
    test: in a scratch copy of the parent a throw-away function evaluated the parent's own expressions -- small / slices / the
    scratch size of gcgcn_gat_bwd, then vec, lds_row, lds, the riding condition, col_base, ncolwg, the grid, the spread constants and
    the RB choice of edge_bwd, then vec / lds / grid of edge_fwd and edge_bcast, att and the LDS sizes of cmp_fwd and cmp_bwd, the
    route and the rowbuf carve of gcgcn_gat_bwd_compact, in that order -- on made-up operand addresses, over these same rows.  A
    launch that carries nothing has RB, col_base, ncolwg and the Spread all 0.  No tolerance, no row left out."""
    import ctypes
    import numpy as np

    def plan(args):
        out = np.full(len(EDGE_PLAN_FIELDS), -7, np.int32)
        _lib.call("gcgcn_debug_edge_plan", *args, out.ctypes.data_as(ctypes.c_void_p))
        return out

    rows = edge_plan_sweep()
    want = np.load(os.path.join(ROOT, "tests", "golden", "edge_plan_parent.npz"))
    assert want["args"].tolist() == [list(r) for r in rows], "the recorded table and edge_plan_sweep list different rows"
    assert want["plan"].shape == (len(rows), len(EDGE_PLAN_FIELDS)) and len(rows) > 2500
    f = {name: k for k, name in enumerate(EDGE_PLAN_FIELDS)}
    wrong = []
    for args, w in zip(rows, want["plan"]):
        got = plan(args)
        if not np.array_equal(got, w):
            diff = {name: (int(w[k]), int(got[k])) for name, k in f.items() if w[k] != got[k]}
            wrong.append(f"{dict(zip(EDGE_PLAN_ARGS, args))}: (want, got) {diff}")
            continue
        ps, compact, B, N = args[:4]
        if ps == 1 and not compact:   # structure of a dense backward launch
            ntile = got[f["sp_na"]]
            assert got[f["grid"]] == B * N + got[f["ngat"]] + ntile + got[f["ncolwg"]], args
            assert (got[f["col_base"]] == 0) == (got[f["ncolwg"]] == 0), args
            assert got[f["col_base"]] in (0, B * N + got[f["ngat"]] + ntile), args
            if got[f["vec"]] == 1 or not got[f["carry_ok"]]:
                assert ntile == 0 and got[f["ncolwg"]] == 0 and got[f["RB"]] == 0, args
            if ntile:
                assert got[f["lds"]] == 0 and got[f["sp_cohort"]] == 256 and got[f["sp_stride"]] % 8 == 0, args
        else:
            assert got[f["grid"]] == B * N, args
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ\n" + "\n".join(wrong[:40])
    # every value of a decision occurs in the table
    cols = {name: set(want["plan"][:, k].tolist()) for name, k in f.items()}
    assert cols["vec"] == {-1, 1, 4} and cols["route"] == {-1, 0, 1, 2} and cols["slices"] == {-1, 1, 4, 8}
    assert cols["lds_ok"] == {-1, 0, 1} and cols["carry_ok"] == {-1, 0, 1} and cols["RB"] == {-1, 0, 1}
    # compact rows stop at D = 512: the hook refuses what cmp_check refuses
    with pytest.raises(RuntimeError, match="compact rows support up to 512"):
        plan((0, 1, 3, 16, EDGE_CMP_MAX_D + 1, 0, 1, 1, 1, 0, 0, 0, 0))


# ---- the attention core's plan ------------------------------------------------------------------------------------------------------
ATTN_PLAN_ARGS = ["bwd", "N", "D", "H", "hook", "chain_attends", "core_done", "misalign", "mha_core"]
ATTN_PLAN_FIELDS = ["route", "kchunk", "fusable", "refused"]
ATTN_ROUTES = {"GEMM": 0, "CORE": 1, "CHAIN": 2, "GROUP": 3, "DONE": 4}


def attn_plan_sweep():
    """The argument rows (ATTN_PLAN_ARGS) of the plan table: graph sizes either side of the core's 64, head widths of 3, 4, 6, 10, 16,
    32, 64, 128 and 192, every combination of the flags."""
    import itertools
    NS = (1, 16, 63, 64, 65, 128)
    DH = ((8, 2), (12, 4), (24, 4), (64, 4), (128, 8), (256, 8), (256, 4), (256, 2), (768, 4), (512, 8), (30, 3))
    assert sorted({D // H for D, H in DH}) == [3, 4, 6, 10, 16, 32, 64, 128, 192]
    return [(bwd, N, D, H, hook, att, done, mis, core)
            for N, (D, H), hook, att, done, mis, core, bwd in itertools.product(NS, DH, (0, 1), (0, 1), (0, 1), (0, 1, 2, 3), (1, 0), (0, 1))]


def test_attn_plan_is_the_decision_the_scattered_predicates_made():
    """gcgcn_debug_attn_plan (the plan functions gcgcn_mha_fwd / _bwd and the hooked gcgcn_gcn_fwd / _bwd call) gives, for every row of
    attn_plan_sweep, the place the code before it ran the attention core in, the head-feature chunk it ran it with, and
    gcgcn_maggc_fusable's answer.  The expected table (tests/golden/attn_plan_parent.npz) was recorded from the PARENT of the commit
    that introduced AttnPlan, not from the code under test: in a scratch copy of the parent a throw-away function evaluated the
    parent's own expressions in the order the entry points evaluated them -- use_mha_core and mha_core_ok of gcgcn_mha_fwd / _bwd
    after core_done; gcgcn_maggc_fusable, then mha_core_ok, then plan.attention of gcgcn_gcn_fwd; gcgcn_maggc_fusable, mha_core_ok,
    mha_chunk, gemm_group_can_carry_mha and gemm_group_mha_chunk of gcgcn_gcn_bwd -- on made-up operand addresses, over these same
    rows.  A hook the parent refused is recorded with the check that refused it (gcgcn_maggc_fusable first: 1, then mha_core_ok's
    alignment: 2; route and chunk -1) and must be refused by the same check (attn_hook_refusal, which the entry points ask).  No tolerance, no row left out."""
    import ctypes
    import numpy as np

    def plan(*args):
        out = np.full(len(ATTN_PLAN_FIELDS), -7, np.int32)
        _lib.call("gcgcn_debug_attn_plan", *args, out.ctypes.data_as(ctypes.c_void_p))
        return [int(v) for v in out]

    rows = attn_plan_sweep()
    want = np.load(os.path.join(ROOT, "tests", "golden", "attn_plan_parent.npz"))
    assert want["args"].tolist() == [list(r) for r in rows], "the recorded table and attn_plan_sweep list different rows"
    assert want["plan"].shape == (len(rows), len(ATTN_PLAN_FIELDS)) and len(rows) == 6 * 11 * 128
    wrong = []
    try:
        for args, w in zip(rows, want["plan"].tolist()):
            _lib.call("gcgcn_set_option", b"mha_core", args[8])
            got = plan(*args[:8])
            if got != w:
                wrong.append(f"{dict(zip(ATTN_PLAN_ARGS, args))}: want {w} got {got}")
    finally:
        _lib.call("gcgcn_set_option", b"mha_core", 1)
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ\n" + "\n".join(wrong[:40])
    # every route, both refusals and both answers of fusable occur in the table; a chunk is 32, 64 or 128 features, or none
    cols = {name: set(want["plan"][:, k].tolist()) for k, name in enumerate(ATTN_PLAN_FIELDS)}
    assert cols["route"] == {-1, *ATTN_ROUTES.values()} and cols["refused"] == {0, 1, 2} and cols["fusable"] == {0, 1}
    assert cols["kchunk"] == {-1, 0, 32, 64, 128}
    # the wide head's backward core is the only hooked route that is a launch: the smallest such width is 68 (chunk 96), 64 still rides
    assert plan(1, 16, 128, 2, 1, 0, 0, 0)[:2] == [ATTN_ROUTES["GROUP"], 64] and plan(1, 16, 136, 2, 1, 0, 0, 0)[:2] == [ATTN_ROUTES["CORE"], 96]


# ---- the plan of the convolution backward's output stage ------------------------------------------------------------------------
OUT_BWD_ARGS = ["fuse", "B", "N", "D", "H", "scratch", "wsum_fwd", "ragged", "odrop", "drop", "dxres_misaligned", "front_reduced"]
OUT_BWD_FIELDS = ["mask", "wsum", "fold", "fold_drop", "head_sum_launch", "dwlin", "col1", "chain_slices", "col2", "back_ready_slices"]
OUT_BWD_MASK = {"NONE": 0, "LAUNCH": 1, "CHAIN": 2}
OUT_BWD_WSUM = {"NONE": 0, "FORWARD": 1, "HERE": 2}
OUT_BWD_FOLD = {"NONE": 0, "ONE_HEAD": 1, "HEADS": 2}
OUT_BWD_DWLIN = {"FRONT": 0, "BACK": 1}
OUT_BWD_COL1 = {"CHAIN": 0, "FRONT": 1, "BACK": 2, "OWN_LAUNCH": 3}
OUT_BWD_COL2 = {"FRONT_REDUCE": 0, "HEAD_SUM_KERNEL": 1, "BACK_LAUNCH": 2, "BACK_REDUCE": 3, "DONE": 4}
OUT_BWD_FOLD_MAX = 2 << 20   # elements of dHO = B N H D up to which the fold pays (out_bwd_plan)


def out_bwd_plan_sweep():
    """The argument rows (OUT_BWD_ARGS) of the plan table: one, 32 and 33 documents (2 B either side of the 64 slices the chain
    may leave), one, two and eight heads, a small block and, at D = 256, the graph sizes that put B N H D just below, exactly on
    and just above the fold threshold (33 documents never land on it: the sizes either side), every combination of the flags.
    Rows with fuse = 1 and scratch = 0 are left out: chain_plan_bwd never fuses without workspace, and gcgcn_gcn_bwd refuses it."""
    import itertools
    rows = []
    for fuse, H, B in itertools.product((0, 1), (1, 2, 8), (1, 32, 33)):
        n_on = OUT_BWD_FOLD_MAX // (B * H * 256)
        sizes = [(16, 64), (n_on, 256), (n_on + 1, 256)] + ([(n_on - 1, 256)] if B * n_on * H * 256 == OUT_BWD_FOLD_MAX else [])
        for (N, D), scratch, rest in itertools.product(sizes, (0, 1), itertools.product((0, 1), repeat=6)):
            if not (fuse and not scratch):
                rows.append((fuse, B, N, D, H, scratch, *rest))
    return rows


def test_out_bwd_plan_is_the_decision_the_inline_code_made():
    """gcgcn_debug_out_bwd_plan (out_bwd_plan, then out_bwd_plan_col2: the two plan functions gcgcn_gcn_bwd calls) gives, for every
    row of out_bwd_plan_sweep, what the code before it decided inline.  The expected table (tests/golden/out_bwd_plan_parent.npz)
    was recorded from the PARENT of the commit that introduced OutBwdPlan, not from the code under test: in a scratch copy of the
    parent a throw-away function evaluated the parent's own expressions over these same rows, in the order gcgcn_gcn_bwd evaluated
    them -- `wsum`, the two mask_rows conditions, fold_hs, the dHO.C / C2 conditions, where dWlin is offered, c.colpart /
    ready_slices, col_later (from front_reduced, as gemm_group reports it), col_pending, and which call received &cr -- on made-up
    operand addresses.  Rows with fuse = 1 and scratch = 0 are not in the sweep (chain_plan_bwd never produces them) and must be
    refused.  No tolerance, no other row left out; every value of every enum occurs."""
    import ctypes
    import numpy as np

    def plan(*args):
        out = np.full(len(OUT_BWD_FIELDS), -7, np.int32)
        _lib.call("gcgcn_debug_out_bwd_plan", *args, out.ctypes.data_as(ctypes.c_void_p))
        return [int(v) for v in out]

    rows = out_bwd_plan_sweep()
    want = np.load(os.path.join(ROOT, "tests", "golden", "out_bwd_plan_parent.npz"))
    assert want["args"].tolist() == [list(r) for r in rows], "the recorded table and out_bwd_plan_sweep list different rows"
    assert want["plan"].shape == (len(rows), len(OUT_BWD_FIELDS)) and len(rows) == 3 * 11 * 64 * (2 + 1)   # heads, (B, size) pairs, flags, (scratch or not) + fused
    elems = {r[1] * r[2] * r[3] * r[4] - OUT_BWD_FOLD_MAX for r in rows}
    assert 0 in elems and min(e for e in elems if e > 0) <= 33 * 8 * 256 and max(e for e in elems if e < 0) >= -33 * 8 * 256
    wrong = [f"{dict(zip(OUT_BWD_ARGS, args))}: want {w} got {plan(*args)}" for args, w in zip(rows, want["plan"].tolist()) if plan(*args) != w]
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ\n" + "\n".join(wrong[:40])
    cols = {name: set(want["plan"][:, k].tolist()) for k, name in enumerate(OUT_BWD_FIELDS)}
    for name, enum in (("mask", OUT_BWD_MASK), ("wsum", OUT_BWD_WSUM), ("fold", OUT_BWD_FOLD), ("dwlin", OUT_BWD_DWLIN),
                       ("col1", OUT_BWD_COL1), ("col2", OUT_BWD_COL2)):
        assert cols[name] == set(enum.values()), name
    assert cols["fold_drop"] == {0, 1} and cols["head_sum_launch"] == {0, 1}
    assert cols["chain_slices"] == {0, 2, 64} and cols["back_ready_slices"] == {0, 2, 64}
    with pytest.raises(Exception, match="without scratch"):    # fuse implies scratch
        plan(1, 2, 16, 64, 4, 0, 0, 0, 0, 0, 0, 0)


# ---- the GEMM launcher's plan ---------------------------------------------------------------------------------------------------
GEMM_WS = 16 << 20   # workspace elements that hold every split of these shapes


def gemm_problem(form, M, N, K, rb=0, batch=1, ws=GEMM_WS, mis=0, lda_off=0):
    """The 13 integers of a problem for gcgcn_debug_gemm_plan: form nn / nt / tn with its natural leading dimensions."""
    a_kc, b_kc = {"nn": (1, 0), "nt": (1, 1), "tn": (0, 0), "tt": (0, 1)}[form]
    return [M, N, K, a_kc, b_kc, (K if a_kc else M) + lda_off, K if b_kc else N, N, batch, 1, rb, ws, mis]


# name -> problem.  The three products of the path in their natural storage forms; the forced split of a long-K row-block problem
# (768 x 768 x 3072: 144 tiles, 96 k-steps) and the same batched (the list is dropped: nb != 1); the smallest interior problem; a mode 2
# list longer than ROWBLK_LIST_MAX; K % 64 != 0 under mode 2; a guarded shape; N % 4 != 0; a 128-tile mode 1 problem (the `small`
# rule) next to a 1024-tile one; mode 2 / mode 1 with the storage form they serve and with one they do not; then workspace absent, too
# small for the chosen split (4 x 256 x 2048 floats), misaligned; the forced split's workspace at exactly 2, 4 and 7 slabs (widen 1,
# 2, 2); A / B misaligned; a leading dimension that is no multiple of 4; a guarded problem with a row-block list; the two refusals.
GEMM_PLAN_CASES = {
    "nt2048x2048x256": gemm_problem("nt", 2048, 2048, 256),
    "nn2048x256x2048": gemm_problem("nn", 2048, 256, 2048),
    "tn256x2048x2048": gemm_problem("tn", 256, 2048, 2048),
    "longK rb1": gemm_problem("nn", 768, 768, 3072, rb=1),
    "longK rb1 batch8": gemm_problem("nn", 768, 768, 3072, rb=1, batch=8),
    "nn64x64x32": gemm_problem("nn", 64, 64, 32),
    "tn64x64x16384 rb2": gemm_problem("tn", 64, 64, 16384, rb=2),
    "tn128x128x96 rb2": gemm_problem("tn", 128, 128, 96, rb=2),
    "nn100x40x50": gemm_problem("nn", 100, 40, 50),
    "nn128x130x64": gemm_problem("nn", 128, 130, 64),
    "128 tiles rb1": gemm_problem("nn", 512, 1024, 256, rb=1),
    "1024 tiles rb1": gemm_problem("nn", 2048, 2048, 256, rb=1),
    "tn rb2": gemm_problem("tn", 256, 2048, 2048, rb=2),
    "nt rb2": gemm_problem("nt", 2048, 2048, 256, rb=2),
    "tn rb1": gemm_problem("tn", 256, 2048, 2048, rb=1),
    "tn no ws": gemm_problem("tn", 256, 2048, 2048, ws=0),
    "tn ws small": gemm_problem("tn", 256, 2048, 2048, ws=1 << 20),
    "tn ws misaligned": gemm_problem("tn", 256, 2048, 2048, mis=4),
    "longK rb1 no ws": gemm_problem("nn", 768, 768, 3072, rb=1, ws=0),
    "longK rb1 ws 2 slabs": gemm_problem("nn", 768, 768, 3072, rb=1, ws=2 * 768 * 768),
    "longK rb1 ws 4 slabs": gemm_problem("nn", 768, 768, 3072, rb=1, ws=4 * 768 * 768),
    "longK rb1 ws 7 slabs": gemm_problem("nn", 768, 768, 3072, rb=1, ws=7 * 768 * 768),
    "nt A misaligned": gemm_problem("nt", 2048, 2048, 256, mis=1),
    "nt B misaligned": gemm_problem("nt", 2048, 2048, 256, mis=2),
    "nn lda + 2": gemm_problem("nn", 2048, 256, 2048, lda_off=2),
    "guarded rb1": gemm_problem("nn", 2048, 2040, 256, rb=1),
    "K = 0": gemm_problem("nn", 64, 64, 0),
    "M * ld = 2^32": gemm_problem("nn", 1 << 21, 2048, 64),
}
GEMM_PLAN_CAPS = [0, 1, 63, 64, 65, 4096, 100000]
GEMM_GROUP_WORK = 1 << 20
# (pair form 5 gemm_dyn_pair / 6 _ww / 7 _xx, problem a, problem b); the count replaces K of a weight gradient (tn), M of the others
GEMM_PAIR_CASES = {
    "wx": (5, gemm_problem("tn", 256, 512, 1), gemm_problem("nn", 1, 256, 512)),
    "wx no ws": (5, gemm_problem("tn", 256, 512, 1, ws=0), gemm_problem("nn", 1, 256, 512)),
    "wx ws misaligned": (5, gemm_problem("tn", 256, 512, 1, mis=4), gemm_problem("nn", 1, 256, 512)),
    "wx x guarded": (5, gemm_problem("tn", 256, 512, 1), gemm_problem("nn", 1, 256, 50)),
    "wx w guarded": (5, gemm_problem("tn", 250, 512, 1), gemm_problem("nn", 1, 256, 512)),
    "wx w stored nt": (5, gemm_problem("nt", 256, 512, 1), gemm_problem("nn", 1, 256, 512)),
    "wx x stored nt": (5, gemm_problem("tn", 256, 512, 1), gemm_problem("nt", 1, 256, 512)),
    "wx w batched": (5, gemm_problem("tn", 256, 512, 1, batch=2), gemm_problem("nn", 1, 256, 512)),
    "wx x B misaligned": (5, gemm_problem("tn", 256, 512, 1), gemm_problem("nn", 1, 256, 512, mis=2)),
    "ww": (6, gemm_problem("tn", 256, 512, 1), gemm_problem("tn", 256, 512, 1)),
    "ww ws 3M": (6, gemm_problem("tn", 256, 512, 1, ws=3 << 20), gemm_problem("tn", 256, 512, 1)),
    "ww shapes differ": (6, gemm_problem("tn", 256, 512, 1), gemm_problem("tn", 256, 256, 1)),
    "ww ws misaligned": (6, gemm_problem("tn", 256, 512, 1, mis=4), gemm_problem("tn", 256, 512, 1)),
    "ww b A misaligned": (6, gemm_problem("tn", 256, 512, 1), gemm_problem("tn", 256, 512, 1, mis=1)),
    "ww b stored nn": (6, gemm_problem("tn", 256, 512, 1), gemm_problem("nn", 256, 512, 1)),
    "ww guarded": (6, gemm_problem("tn", 256, 500, 1), gemm_problem("tn", 256, 500, 1)),
    "xx": (7, gemm_problem("nn", 1, 256, 512), gemm_problem("nn", 1, 128, 96)),
    "xx b guarded": (7, gemm_problem("nn", 1, 256, 512), gemm_problem("nn", 1, 100, 96)),
    "xx a K guarded": (7, gemm_problem("nn", 1, 256, 50), gemm_problem("nn", 1, 128, 96)),
    "xx a A misaligned": (7, gemm_problem("nn", 1, 256, 512, mis=1), gemm_problem("nn", 1, 128, 96)),
    "xx b stored tn": (7, gemm_problem("nn", 1, 256, 512), gemm_problem("tn", 1, 128, 96)),
    "xx b batched": (7, gemm_problem("nn", 1, 256, 512), gemm_problem("nn", 1, 128, 96, batch=2)),
}


def gemm_plan_code(o):
    """Twelve integers of a plan as I|G (interior | guarded) splits / ksplit, then what differs from the usual: w widen (1), r kept
    row-block mode (0), v vecA vecB (11); t tiles, R (a reduce launch follows), Z (the zero-fill launch), g grid (0); x: refused."""
    if o[0] != 1:
        return "x"
    return (f"{'GI'[o[1]]}{o[2]}/{o[3]}" + (f"w{o[4]}" if o[4] != 1 else "") + (f"r{o[5]}" if o[5] else "") +
            (f"v{o[6]}{o[7]}" if (o[6], o[7]) != (1, 1) else "") + f"t{o[8]}" + ("R" if o[9] else "") + ("Z" if o[10] else "") +
            (f"g{o[11]}" if o[11] else ""))


def gemm_plan_table(plan, set_option):
    """plan(form, prob_a, prob_b, splits, group_work, cap) -> 26 ints.  Per case and split_widen setting three lines: the host-side
    forms (single launch with requested splits 0, 1, 4; member of a group launch of GEMM_GROUP_WORK tile-k-steps; parking), device-side
    M per cap, device-side K per cap.  Then per pair case and setting one line: per cap F gridW (fused) or 2 (two gemm_dyn calls) and
    the two problems' plans."""
    lines, plans = [], 0
    try:
        for name, prob in GEMM_PLAN_CASES.items():
            for sw in (0, 1):
                set_option("split_widen", sw)
                host = [plan(0, prob, None, s, 0, 0) for s in (0, 1, 4)] + [plan(1, prob, None, 0, GEMM_GROUP_WORK, 0), plan(2, prob, None, 0, 0, 0)]
                lines.append(f"{name} sw{sw} host: " + " ".join(gemm_plan_code(o) for o in host))
                for form, label in ((3, "dynM"), (4, "dynK")):
                    lines.append(f"{name} sw{sw} {label}: " + " ".join(gemm_plan_code(plan(form, prob, None, 0, 0, cap)) for cap in GEMM_PLAN_CAPS))
                plans += 5 + 2 * len(GEMM_PLAN_CAPS)
        for name, (form, a, b) in GEMM_PAIR_CASES.items():
            for sw in (0, 1):
                set_option("split_widen", sw)
                codes = []
                for cap in GEMM_PLAN_CAPS:
                    o = plan(form, a, b, 0, 0, cap)
                    codes.append((f"F{o[25]}" if o[24] else "2") + "," + gemm_plan_code(o[:12]) + "," + gemm_plan_code(o[12:24]))
                    plans += 1
                lines.append(f"pair {name} sw{sw}: " + " ".join(codes))
    finally:
        set_option("split_widen", OPTION_DEFAULTS["split_widen"])
    return lines, plans


# Recorded from the PARENT of the commit that introduced gemm_plan, not from the code under test: in a scratch copy of the parent a
# throw-away function called the parent's own prepare() and evaluated, in the order each caller did, the `al` expressions of gemm,
# gemm_group and gemm_defer, gemm_dyn's `al`, split factor, workspace test and grid, and the three pair functions' `ok` chains, split
# factors, workspace tests and grids (a pair that falls back: gemm_dyn's on the two original problems), on the operand addresses
# gcgcn_debug_gemm_plan makes up, and gemm_plan_table printed this.  Rows that take / do not take each branch:
#   prepare() refuses: "K = 0", "M * ld = 2^32" / every other case;  splits == 0 picks: host column 1 / columns 2, 3 (requested 1, 4)
#   the forced split of a long-K row-block problem: "longK rb1 sw1" host column 4 (2/1536) / sw0 (split_widen), "1024 tiles rb1" (K
#     short), "longK rb1 batch8" (1152 tiles); applied before the list is dropped: "tn rb1 sw1" column 4 stays split, list gone
#   the workspace rule unsplits: "tn no ws", "tn ws small", "tn ws misaligned", "nn128x130x64" (N % 4), "tn128x128x96 rb2" column 3
#     (K % (4 BK)) / "tn256x2048x2048"
#   the list is kept: "1024 tiles rb1" (mode 1), "tn rb2" (mode 2) / dropped: "guarded rb1" (not interior), "longK rb1 batch8" (nb),
#     "tn rb1", "nt rb2" (storage form), "tn128x128x96 rb2" (K % 64), "tn64x64x16384 rb2" (list too long; its dynK caps <= 4096 keep it)
#   small: "128 tiles rb1" columns 1, 5 (single launch, parking: dense) / column 4 (member: kept), "longK rb1" column 1 (288 workgroups)
#   widen: "longK rb1 ws 2 / 4 / 7 slabs sw1" column 4 (1, 2, 2), "longK rb1 sw1" (4) / the same under sw0
#   gemm_dyn: interior I / guarded G; the split factor is want ("nn2048x256x2048" cap 4096: 8), most ("nn64x64x32" cap 4096: 16), 1
#     (caps < 256) or the limit of 64 (cap 100000); its workspace test fails: "tn no ws" dynK (Z: the zero-fill launch) /
#     "tn256x2048x2048"; batched: "longK rb1 batch8" refused
#   the pairs' ok chains: batch ("wx w batched", "xx b batched"), storage forms ("wx w stored nt", "wx x stored nt", "ww b stored nn",
#     "xx b stored tn"), equal shapes ("ww shapes differ"), interior ("wx x guarded", "wx w guarded", "wx x B misaligned", "ww b A
#     misaligned", "ww guarded", "xx b guarded", "xx a K guarded", "xx a A misaligned"), splits > 1 (caps < 512), the workspace ("wx no
#     ws", "wx ws misaligned", "ww ws 3M": holds one problem's slabs, not both, "ww ws misaligned") / "wx", "ww", "xx" at caps >= 4096
GEMM_PLAN_EXPECTED = """
nt2048x2048x256 sw0 host: I1/256t1024 I1/256t1024 I4/64t1024R I1/256t1024 I1/256t1024
nt2048x2048x256 sw0 dynM: I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t64g64 I1/256t2048g1024 I1/256t50016g1024
nt2048x2048x256 sw0 dynK: I1/64t1024Zg1024 I1/64t1024Zg1024 I1/64t1024Zg1024 I1/64t1024Zg1024 I1/128t1024Zg1024 I1/4096t1024Zg1024 I1/100032t1024Zg1024
nt2048x2048x256 sw1 host: I1/256t1024 I1/256t1024 I4/64t1024R I1/256t1024 I1/256t1024
nt2048x2048x256 sw1 dynM: I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t64g64 I1/256t2048g1024 I1/256t50016g1024
nt2048x2048x256 sw1 dynK: I1/64t1024Zg1024 I1/64t1024Zg1024 I1/64t1024Zg1024 I1/64t1024Zg1024 I1/128t1024Zg1024 I1/4096t1024Zg1024 I1/100032t1024Zg1024
nn2048x256x2048 sw0 host: I4/512t128R I1/2048t128 I4/512t128R I1/2048t128 I1/2048t128
nn2048x256x2048 sw0 dynM: I1/2048t4g4 I1/2048t4g4 I1/2048t4g4 I1/2048t4g4 I1/2048t8g8 I1/2048t256g256 I1/2048t6252g1024
nn2048x256x2048 sw0 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I8/4096t128Rg1024 I8/100032t128Rg1024
nn2048x256x2048 sw1 host: I4/512t128R I1/2048t128 I4/512t128R I1/2048t128 I1/2048t128
nn2048x256x2048 sw1 dynM: I1/2048t4g4 I1/2048t4g4 I1/2048t4g4 I1/2048t4g4 I1/2048t8g8 I1/2048t256g256 I1/2048t6252g1024
nn2048x256x2048 sw1 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I8/4096t128Rg1024 I8/100032t128Rg1024
tn256x2048x2048 sw0 host: I4/512t128R I1/2048t128 I4/512t128R I1/2048t128 I1/2048t128
tn256x2048x2048 sw0 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn256x2048x2048 sw0 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I8/4096t128Rg1024 I8/100032t128Rg1024
tn256x2048x2048 sw1 host: I4/512t128R I1/2048t128 I4/512t128R I1/2048t128 I1/2048t128
tn256x2048x2048 sw1 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn256x2048x2048 sw1 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I8/4096t128Rg1024 I8/100032t128Rg1024
longK rb1 sw0 host: I4/768r1t144R I1/3072t144 I4/768r1t144R I1/3072r1t144 I1/3072t144
longK rb1 sw0 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 sw0 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I8/4096t144Rg1024 I8/100032t144Rg1024
longK rb1 sw1 host: I4/768w4r1t144R I1/3072t144 I4/768w4r1t144R I2/1536w4r1t144R I1/3072t144
longK rb1 sw1 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 sw1 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I8/4096t144Rg1024 I8/100032t144Rg1024
longK rb1 batch8 sw0 host: I1/3072t1152 I1/3072t1152 I1/3072t1152 I1/3072t1152 I1/3072t1152
longK rb1 batch8 sw0 dynM: x x x x x x x
longK rb1 batch8 sw0 dynK: x x x x x x x
longK rb1 batch8 sw1 host: I1/3072t1152 I1/3072t1152 I1/3072t1152 I1/3072t1152 I1/3072t1152
longK rb1 batch8 sw1 dynM: x x x x x x x
longK rb1 batch8 sw1 dynK: x x x x x x x
nn64x64x32 sw0 host: I1/32t1 I1/32t1 I1/32t1 I1/32t1 I1/32t1
nn64x64x32 sw0 dynM: I1/32t1g1 I1/32t1g1 I1/32t1g1 I1/32t1g1 I1/32t2g2 I1/32t64g64 I1/32t1563g1024
nn64x64x32 sw0 dynK: I1/64t1Zg1 I1/64t1Zg1 I1/64t1Zg1 I1/64t1Zg1 I1/128t1Zg1 I16/4096t1Rg16 I64/100032t1Rg64
nn64x64x32 sw1 host: I1/32t1 I1/32t1 I1/32t1 I1/32t1 I1/32t1
nn64x64x32 sw1 dynM: I1/32t1g1 I1/32t1g1 I1/32t1g1 I1/32t1g1 I1/32t2g2 I1/32t64g64 I1/32t1563g1024
nn64x64x32 sw1 dynK: I1/64t1Zg1 I1/64t1Zg1 I1/64t1Zg1 I1/64t1Zg1 I1/128t1Zg1 I16/4096t1Rg16 I64/100032t1Rg64
tn64x64x16384 rb2 sw0 host: I16/1024t1R I1/16384t1 I4/4096t1R I1/16384t1 I1/16384t1
tn64x64x16384 rb2 sw0 dynM: I1/16384t1g1 I1/16384t1g1 I1/16384t1g1 I1/16384t1g1 I1/16384t2g2 I1/16384t64g64 I1/16384t1563g1024
tn64x64x16384 rb2 sw0 dynK: I1/64r2t1Zg1 I1/64r2t1Zg1 I1/64r2t1Zg1 I1/64r2t1Zg1 I1/128r2t1Zg1 I16/4096r2t1Rg16 I64/100032t1Rg64
tn64x64x16384 rb2 sw1 host: I16/1024t1R I1/16384t1 I4/4096t1R I1/16384t1 I1/16384t1
tn64x64x16384 rb2 sw1 dynM: I1/16384t1g1 I1/16384t1g1 I1/16384t1g1 I1/16384t1g1 I1/16384t2g2 I1/16384t64g64 I1/16384t1563g1024
tn64x64x16384 rb2 sw1 dynK: I1/64r2t1Zg1 I1/64r2t1Zg1 I1/64r2t1Zg1 I1/64r2t1Zg1 I1/128r2t1Zg1 I16/4096r2t1Rg16 I64/100032t1Rg64
tn128x128x96 rb2 sw0 host: I1/96t4 I1/96t4 I1/96t4 I1/96t4 I1/96t4
tn128x128x96 rb2 sw0 dynM: I1/96t2g2 I1/96t2g2 I1/96t2g2 I1/96t2g2 I1/96t4g4 I1/96t128g128 I1/96t3126g1024
tn128x128x96 rb2 sw0 dynK: I1/64r2t4Zg4 I1/64r2t4Zg4 I1/64r2t4Zg4 I1/64r2t4Zg4 I1/128r2t4Zg4 I16/4096r2t4Rg64 I64/100032t4Rg256
tn128x128x96 rb2 sw1 host: I1/96t4 I1/96t4 I1/96t4 I1/96t4 I1/96t4
tn128x128x96 rb2 sw1 dynM: I1/96t2g2 I1/96t2g2 I1/96t2g2 I1/96t2g2 I1/96t4g4 I1/96t128g128 I1/96t3126g1024
tn128x128x96 rb2 sw1 dynK: I1/64r2t4Zg4 I1/64r2t4Zg4 I1/64r2t4Zg4 I1/64r2t4Zg4 I1/128r2t4Zg4 I16/4096r2t4Rg64 I64/100032t4Rg256
nn100x40x50 sw0 host: G1/50v01t2 G1/50v01t2 G1/50v01t2 G1/50v01t2 G1/50v01t2
nn100x40x50 sw0 dynM: G1/50v01t1g1 G1/50v01t1g1 G1/50v01t1g1 G1/50v01t1g1 G1/50v01t2g2 G1/50v01t64g64 G1/50v01t1563g1024
nn100x40x50 sw0 dynK: G1/64v01t2Zg2 G1/64v01t2Zg2 G1/64v01t2Zg2 G1/64v01t2Zg2 G1/128v01t2Zg2 G16/4096v01t2Rg32 G64/100032v01t2Rg128
nn100x40x50 sw1 host: G1/50v01t2 G1/50v01t2 G1/50v01t2 G1/50v01t2 G1/50v01t2
nn100x40x50 sw1 dynM: G1/50v01t1g1 G1/50v01t1g1 G1/50v01t1g1 G1/50v01t1g1 G1/50v01t2g2 G1/50v01t64g64 G1/50v01t1563g1024
nn100x40x50 sw1 dynK: G1/64v01t2Zg2 G1/64v01t2Zg2 G1/64v01t2Zg2 G1/64v01t2Zg2 G1/128v01t2Zg2 G16/4096v01t2Rg32 G64/100032v01t2Rg128
nn128x130x64 sw0 host: G1/64v10t6 G1/64v10t6 G1/64v10t6 G1/64v10t6 G1/64v10t6
nn128x130x64 sw0 dynM: G1/64v10t3g3 G1/64v10t3g3 G1/64v10t3g3 G1/64v10t3g3 G1/64v10t6g6 G1/64v10t192g192 G1/64v10t4689g1024
nn128x130x64 sw0 dynK: G1/64v10t6Zg6 G1/64v10t6Zg6 G1/64v10t6Zg6 G1/64v10t6Zg6 G1/128v10t6Zg6 G1/4096v10t6Zg6 G1/100032v10t6Zg6
nn128x130x64 sw1 host: G1/64v10t6 G1/64v10t6 G1/64v10t6 G1/64v10t6 G1/64v10t6
nn128x130x64 sw1 dynM: G1/64v10t3g3 G1/64v10t3g3 G1/64v10t3g3 G1/64v10t3g3 G1/64v10t6g6 G1/64v10t192g192 G1/64v10t4689g1024
nn128x130x64 sw1 dynK: G1/64v10t6Zg6 G1/64v10t6Zg6 G1/64v10t6Zg6 G1/64v10t6Zg6 G1/128v10t6Zg6 G1/4096v10t6Zg6 G1/100032v10t6Zg6
128 tiles rb1 sw0 host: I1/256t128 I1/256t128 I4/64r1t128R I1/256r1t128 I1/256t128
128 tiles rb1 sw0 dynM: I1/256t16g16 I1/256t16g16 I1/256t16g16 I1/256t16g16 I1/256t32g32 I1/256r1t1024g1024 I1/256r1t25008g1024
128 tiles rb1 sw0 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I8/4096t128Rg1024 I8/100032t128Rg1024
128 tiles rb1 sw1 host: I1/256t128 I1/256t128 I4/64w4r1t128R I1/256r1t128 I1/256t128
128 tiles rb1 sw1 dynM: I1/256t16g16 I1/256t16g16 I1/256t16g16 I1/256t16g16 I1/256t32g32 I1/256r1t1024g1024 I1/256r1t25008g1024
128 tiles rb1 sw1 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I8/4096t128Rg1024 I8/100032t128Rg1024
1024 tiles rb1 sw0 host: I1/256r1t1024 I1/256r1t1024 I4/64r1t1024R I1/256r1t1024 I1/256r1t1024
1024 tiles rb1 sw0 dynM: I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t64g64 I1/256r1t2048g1024 I1/256r1t50016g1024
1024 tiles rb1 sw0 dynK: I1/64r1t1024Zg1024 I1/64r1t1024Zg1024 I1/64r1t1024Zg1024 I1/64r1t1024Zg1024 I1/128r1t1024Zg1024 I1/4096r1t1024Zg1024 I1/100032r1t1024Zg1024
1024 tiles rb1 sw1 host: I1/256r1t1024 I1/256r1t1024 I4/64r1t1024R I1/256r1t1024 I1/256r1t1024
1024 tiles rb1 sw1 dynM: I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t64g64 I1/256r1t2048g1024 I1/256r1t50016g1024
1024 tiles rb1 sw1 dynK: I1/64r1t1024Zg1024 I1/64r1t1024Zg1024 I1/64r1t1024Zg1024 I1/64r1t1024Zg1024 I1/128r1t1024Zg1024 I1/4096r1t1024Zg1024 I1/100032r1t1024Zg1024
tn rb2 sw0 host: I4/512r2t128R I1/2048r2t128 I4/512r2t128R I1/2048r2t128 I1/2048r2t128
tn rb2 sw0 dynM: I1/2048r2t32g32 I1/2048r2t32g32 I1/2048r2t32g32 I1/2048r2t32g32 I1/2048r2t64g64 I1/2048r2t2048g1024 I1/2048r2t50016g1024
tn rb2 sw0 dynK: I1/64r2t128Zg128 I1/64r2t128Zg128 I1/64r2t128Zg128 I1/64r2t128Zg128 I1/128r2t128Zg128 I8/4096r2t128Rg1024 I8/100032t128Rg1024
tn rb2 sw1 host: I4/512r2t128R I1/2048r2t128 I4/512r2t128R I1/2048r2t128 I1/2048r2t128
tn rb2 sw1 dynM: I1/2048r2t32g32 I1/2048r2t32g32 I1/2048r2t32g32 I1/2048r2t32g32 I1/2048r2t64g64 I1/2048r2t2048g1024 I1/2048r2t50016g1024
tn rb2 sw1 dynK: I1/64r2t128Zg128 I1/64r2t128Zg128 I1/64r2t128Zg128 I1/64r2t128Zg128 I1/128r2t128Zg128 I8/4096r2t128Rg1024 I8/100032t128Rg1024
nt rb2 sw0 host: I1/256t1024 I1/256t1024 I4/64t1024R I1/256t1024 I1/256t1024
nt rb2 sw0 dynM: I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t64g64 I1/256t2048g1024 I1/256t50016g1024
nt rb2 sw0 dynK: I1/64t1024Zg1024 I1/64t1024Zg1024 I1/64t1024Zg1024 I1/64t1024Zg1024 I1/128t1024Zg1024 I1/4096t1024Zg1024 I1/100032t1024Zg1024
nt rb2 sw1 host: I1/256t1024 I1/256t1024 I4/64t1024R I1/256t1024 I1/256t1024
nt rb2 sw1 dynM: I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t32g32 I1/256t64g64 I1/256t2048g1024 I1/256t50016g1024
nt rb2 sw1 dynK: I1/64t1024Zg1024 I1/64t1024Zg1024 I1/64t1024Zg1024 I1/64t1024Zg1024 I1/128t1024Zg1024 I1/4096t1024Zg1024 I1/100032t1024Zg1024
tn rb1 sw0 host: I4/512t128R I1/2048t128 I4/512t128R I1/2048t128 I1/2048t128
tn rb1 sw0 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn rb1 sw0 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I8/4096t128Rg1024 I8/100032t128Rg1024
tn rb1 sw1 host: I4/512t128R I1/2048t128 I4/512t128R I2/1024t128R I1/2048t128
tn rb1 sw1 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn rb1 sw1 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I8/4096t128Rg1024 I8/100032t128Rg1024
tn no ws sw0 host: I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128
tn no ws sw0 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn no ws sw0 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I1/4096t128Zg128 I1/100032t128Zg128
tn no ws sw1 host: I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128
tn no ws sw1 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn no ws sw1 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I1/4096t128Zg128 I1/100032t128Zg128
tn ws small sw0 host: I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128
tn ws small sw0 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn ws small sw0 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I1/4096t128Zg128 I1/100032t128Zg128
tn ws small sw1 host: I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128
tn ws small sw1 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn ws small sw1 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I1/4096t128Zg128 I1/100032t128Zg128
tn ws misaligned sw0 host: I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128
tn ws misaligned sw0 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn ws misaligned sw0 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I1/4096t128Zg128 I1/100032t128Zg128
tn ws misaligned sw1 host: I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128 I1/2048t128
tn ws misaligned sw1 dynM: I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t32g32 I1/2048t64g64 I1/2048t2048g1024 I1/2048t50016g1024
tn ws misaligned sw1 dynK: I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/64t128Zg128 I1/128t128Zg128 I1/4096t128Zg128 I1/100032t128Zg128
longK rb1 no ws sw0 host: I1/3072t144 I1/3072t144 I1/3072t144 I1/3072r1t144 I1/3072t144
longK rb1 no ws sw0 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 no ws sw0 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I1/4096t144Zg144 I1/100032t144Zg144
longK rb1 no ws sw1 host: I1/3072t144 I1/3072t144 I1/3072t144 I1/3072r1t144 I1/3072t144
longK rb1 no ws sw1 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 no ws sw1 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I1/4096t144Zg144 I1/100032t144Zg144
longK rb1 ws 2 slabs sw0 host: I1/3072t144 I1/3072t144 I1/3072t144 I1/3072r1t144 I1/3072t144
longK rb1 ws 2 slabs sw0 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 ws 2 slabs sw0 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I1/4096t144Zg144 I1/100032t144Zg144
longK rb1 ws 2 slabs sw1 host: I1/3072t144 I1/3072t144 I1/3072t144 I2/1536r1t144R I1/3072t144
longK rb1 ws 2 slabs sw1 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 ws 2 slabs sw1 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I1/4096t144Zg144 I1/100032t144Zg144
longK rb1 ws 4 slabs sw0 host: I4/768r1t144R I1/3072t144 I4/768r1t144R I1/3072r1t144 I1/3072t144
longK rb1 ws 4 slabs sw0 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 ws 4 slabs sw0 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I1/4096t144Zg144 I1/100032t144Zg144
longK rb1 ws 4 slabs sw1 host: I4/768r1t144R I1/3072t144 I4/768r1t144R I2/1536w2r1t144R I1/3072t144
longK rb1 ws 4 slabs sw1 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 ws 4 slabs sw1 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I1/4096t144Zg144 I1/100032t144Zg144
longK rb1 ws 7 slabs sw0 host: I4/768r1t144R I1/3072t144 I4/768r1t144R I1/3072r1t144 I1/3072t144
longK rb1 ws 7 slabs sw0 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 ws 7 slabs sw0 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I1/4096t144Zg144 I1/100032t144Zg144
longK rb1 ws 7 slabs sw1 host: I4/768r1t144R I1/3072t144 I4/768r1t144R I2/1536w2r1t144R I1/3072t144
longK rb1 ws 7 slabs sw1 dynM: I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t12g12 I1/3072t24g24 I1/3072r1t768g768 I1/3072r1t18756g1024
longK rb1 ws 7 slabs sw1 dynK: I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/64t144Zg144 I1/128t144Zg144 I1/4096t144Zg144 I1/100032t144Zg144
nt A misaligned sw0 host: G1/256v01t1024 G1/256v01t1024 G4/64v01t1024R G1/256v01t1024 G1/256v01t1024
nt A misaligned sw0 dynM: G1/256v01t32g32 G1/256v01t32g32 G1/256v01t32g32 G1/256v01t32g32 G1/256v01t64g64 G1/256v01t2048g1024 G1/256v01t50016g1024
nt A misaligned sw0 dynK: G1/64v01t1024Zg1024 G1/64v01t1024Zg1024 G1/64v01t1024Zg1024 G1/64v01t1024Zg1024 G1/128v01t1024Zg1024 G1/4096v01t1024Zg1024 G1/100032v01t1024Zg1024
nt A misaligned sw1 host: G1/256v01t1024 G1/256v01t1024 G4/64v01t1024R G1/256v01t1024 G1/256v01t1024
nt A misaligned sw1 dynM: G1/256v01t32g32 G1/256v01t32g32 G1/256v01t32g32 G1/256v01t32g32 G1/256v01t64g64 G1/256v01t2048g1024 G1/256v01t50016g1024
nt A misaligned sw1 dynK: G1/64v01t1024Zg1024 G1/64v01t1024Zg1024 G1/64v01t1024Zg1024 G1/64v01t1024Zg1024 G1/128v01t1024Zg1024 G1/4096v01t1024Zg1024 G1/100032v01t1024Zg1024
nt B misaligned sw0 host: G1/256v10t1024 G1/256v10t1024 G4/64v10t1024R G1/256v10t1024 G1/256v10t1024
nt B misaligned sw0 dynM: G1/256v10t32g32 G1/256v10t32g32 G1/256v10t32g32 G1/256v10t32g32 G1/256v10t64g64 G1/256v10t2048g1024 G1/256v10t50016g1024
nt B misaligned sw0 dynK: G1/64v10t1024Zg1024 G1/64v10t1024Zg1024 G1/64v10t1024Zg1024 G1/64v10t1024Zg1024 G1/128v10t1024Zg1024 G1/4096v10t1024Zg1024 G1/100032v10t1024Zg1024
nt B misaligned sw1 host: G1/256v10t1024 G1/256v10t1024 G4/64v10t1024R G1/256v10t1024 G1/256v10t1024
nt B misaligned sw1 dynM: G1/256v10t32g32 G1/256v10t32g32 G1/256v10t32g32 G1/256v10t32g32 G1/256v10t64g64 G1/256v10t2048g1024 G1/256v10t50016g1024
nt B misaligned sw1 dynK: G1/64v10t1024Zg1024 G1/64v10t1024Zg1024 G1/64v10t1024Zg1024 G1/64v10t1024Zg1024 G1/128v10t1024Zg1024 G1/4096v10t1024Zg1024 G1/100032v10t1024Zg1024
nn lda + 2 sw0 host: G4/512v01t128R G1/2048v01t128 G4/512v01t128R G1/2048v01t128 G1/2048v01t128
nn lda + 2 sw0 dynM: G1/2048v01t4g4 G1/2048v01t4g4 G1/2048v01t4g4 G1/2048v01t4g4 G1/2048v01t8g8 G1/2048v01t256g256 G1/2048v01t6252g1024
nn lda + 2 sw0 dynK: G1/64v01t128Zg128 G1/64v01t128Zg128 G1/64v01t128Zg128 G1/64v01t128Zg128 G1/128v01t128Zg128 G8/4096v01t128Rg1024 G8/100032v01t128Rg1024
nn lda + 2 sw1 host: G4/512v01t128R G1/2048v01t128 G4/512v01t128R G1/2048v01t128 G1/2048v01t128
nn lda + 2 sw1 dynM: G1/2048v01t4g4 G1/2048v01t4g4 G1/2048v01t4g4 G1/2048v01t4g4 G1/2048v01t8g8 G1/2048v01t256g256 G1/2048v01t6252g1024
nn lda + 2 sw1 dynK: G1/64v01t128Zg128 G1/64v01t128Zg128 G1/64v01t128Zg128 G1/64v01t128Zg128 G1/128v01t128Zg128 G8/4096v01t128Rg1024 G8/100032v01t128Rg1024
guarded rb1 sw0 host: G1/256t1024 G1/256t1024 G4/64t1024R G1/256t1024 G1/256t1024
guarded rb1 sw0 dynM: G1/256t32g32 G1/256t32g32 G1/256t32g32 G1/256t32g32 G1/256t64g64 G1/256t2048g1024 G1/256t50016g1024
guarded rb1 sw0 dynK: G1/64t1024Zg1024 G1/64t1024Zg1024 G1/64t1024Zg1024 G1/64t1024Zg1024 G1/128t1024Zg1024 G1/4096t1024Zg1024 G1/100032t1024Zg1024
guarded rb1 sw1 host: G1/256t1024 G1/256t1024 G4/64t1024R G1/256t1024 G1/256t1024
guarded rb1 sw1 dynM: G1/256t32g32 G1/256t32g32 G1/256t32g32 G1/256t32g32 G1/256t64g64 G1/256t2048g1024 G1/256t50016g1024
guarded rb1 sw1 dynK: G1/64t1024Zg1024 G1/64t1024Zg1024 G1/64t1024Zg1024 G1/64t1024Zg1024 G1/128t1024Zg1024 G1/4096t1024Zg1024 G1/100032t1024Zg1024
K = 0 sw0 host: x x x x x
K = 0 sw0 dynM: x x x x x x x
K = 0 sw0 dynK: I1/64t1Zg1 I1/64t1Zg1 I1/64t1Zg1 I1/64t1Zg1 I1/128t1Zg1 I16/4096t1Rg16 I64/100032t1Rg64
K = 0 sw1 host: x x x x x
K = 0 sw1 dynM: x x x x x x x
K = 0 sw1 dynK: I1/64t1Zg1 I1/64t1Zg1 I1/64t1Zg1 I1/64t1Zg1 I1/128t1Zg1 I16/4096t1Rg16 I64/100032t1Rg64
M * ld = 2^32 sw0 host: x x x x x
M * ld = 2^32 sw0 dynM: I1/64t32g32 I1/64t32g32 I1/64t32g32 I1/64t32g32 I1/64t64g64 I1/64t2048g1024 I1/64t50016g1024
M * ld = 2^32 sw0 dynK: x x x x x x x
M * ld = 2^32 sw1 host: x x x x x
M * ld = 2^32 sw1 dynM: I1/64t32g32 I1/64t32g32 I1/64t32g32 I1/64t32g32 I1/64t64g64 I1/64t2048g1024 I1/64t50016g1024
M * ld = 2^32 sw1 dynK: x x x x x x x
pair wx sw0: 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/128t32Zg32,I1/512t8g8 F512,I16/4096t32Rg512,I1/512t256g256 F1024,I32/100032t32Rg1024,I1/512t6252g1024
pair wx sw1: 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/128t32Zg32,I1/512t8g8 F512,I16/4096t32Rg512,I1/512t256g256 F1024,I32/100032t32Rg1024,I1/512t6252g1024
pair wx no ws sw0: 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/128t32Zg32,I1/512t8g8 2,I1/4096t32Zg32,I1/512t256g256 2,I1/100032t32Zg32,I1/512t6252g1024
pair wx no ws sw1: 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/128t32Zg32,I1/512t8g8 2,I1/4096t32Zg32,I1/512t256g256 2,I1/100032t32Zg32,I1/512t6252g1024
pair wx ws misaligned sw0: 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/128t32Zg32,I1/512t8g8 2,I1/4096t32Zg32,I1/512t256g256 2,I1/100032t32Zg32,I1/512t6252g1024
pair wx ws misaligned sw1: 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/128t32Zg32,I1/512t8g8 2,I1/4096t32Zg32,I1/512t256g256 2,I1/100032t32Zg32,I1/512t6252g1024
pair wx x guarded sw0: 2,I1/64t32Zg32,G1/50v01t4g4 2,I1/64t32Zg32,G1/50v01t4g4 2,I1/64t32Zg32,G1/50v01t4g4 2,I1/64t32Zg32,G1/50v01t4g4 2,I1/128t32Zg32,G1/50v01t8g8 2,I16/4096t32Rg512,G1/50v01t256g256 2,I32/100032t32Rg1024,G1/50v01t6252g1024
pair wx x guarded sw1: 2,I1/64t32Zg32,G1/50v01t4g4 2,I1/64t32Zg32,G1/50v01t4g4 2,I1/64t32Zg32,G1/50v01t4g4 2,I1/64t32Zg32,G1/50v01t4g4 2,I1/128t32Zg32,G1/50v01t8g8 2,I16/4096t32Rg512,G1/50v01t256g256 2,I32/100032t32Rg1024,G1/50v01t6252g1024
pair wx w guarded sw0: 2,G1/64v01t32Zg32,I1/512t4g4 2,G1/64v01t32Zg32,I1/512t4g4 2,G1/64v01t32Zg32,I1/512t4g4 2,G1/64v01t32Zg32,I1/512t4g4 2,G1/128v01t32Zg32,I1/512t8g8 2,G16/4096v01t32Rg512,I1/512t256g256 2,G32/100032v01t32Rg1024,I1/512t6252g1024
pair wx w guarded sw1: 2,G1/64v01t32Zg32,I1/512t4g4 2,G1/64v01t32Zg32,I1/512t4g4 2,G1/64v01t32Zg32,I1/512t4g4 2,G1/64v01t32Zg32,I1/512t4g4 2,G1/128v01t32Zg32,I1/512t8g8 2,G16/4096v01t32Rg512,I1/512t256g256 2,G32/100032v01t32Rg1024,I1/512t6252g1024
pair wx w stored nt sw0: 2,G1/64v00t32Zg32,I1/512t4g4 2,G1/64v00t32Zg32,I1/512t4g4 2,G1/64v00t32Zg32,I1/512t4g4 2,G1/64v00t32Zg32,I1/512t4g4 2,G1/128v00t32Zg32,I1/512t8g8 2,G16/4096v00t32Rg512,I1/512t256g256 2,G32/100032v00t32Rg1024,I1/512t6252g1024
pair wx w stored nt sw1: 2,G1/64v00t32Zg32,I1/512t4g4 2,G1/64v00t32Zg32,I1/512t4g4 2,G1/64v00t32Zg32,I1/512t4g4 2,G1/64v00t32Zg32,I1/512t4g4 2,G1/128v00t32Zg32,I1/512t8g8 2,G16/4096v00t32Rg512,I1/512t256g256 2,G32/100032v00t32Rg1024,I1/512t6252g1024
pair wx x stored nt sw0: 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/128t32Zg32,I1/512t8g8 2,I16/4096t32Rg512,I1/512t256g256 2,I32/100032t32Rg1024,I1/512t6252g1024
pair wx x stored nt sw1: 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/64t32Zg32,I1/512t4g4 2,I1/128t32Zg32,I1/512t8g8 2,I16/4096t32Rg512,I1/512t256g256 2,I32/100032t32Rg1024,I1/512t6252g1024
pair wx w batched sw0: 2,x,I1/512t4g4 2,x,I1/512t4g4 2,x,I1/512t4g4 2,x,I1/512t4g4 2,x,I1/512t8g8 2,x,I1/512t256g256 2,x,I1/512t6252g1024
pair wx w batched sw1: 2,x,I1/512t4g4 2,x,I1/512t4g4 2,x,I1/512t4g4 2,x,I1/512t4g4 2,x,I1/512t8g8 2,x,I1/512t256g256 2,x,I1/512t6252g1024
pair wx x B misaligned sw0: 2,I1/64t32Zg32,G1/512v10t4g4 2,I1/64t32Zg32,G1/512v10t4g4 2,I1/64t32Zg32,G1/512v10t4g4 2,I1/64t32Zg32,G1/512v10t4g4 2,I1/128t32Zg32,G1/512v10t8g8 2,I16/4096t32Rg512,G1/512v10t256g256 2,I32/100032t32Rg1024,G1/512v10t6252g1024
pair wx x B misaligned sw1: 2,I1/64t32Zg32,G1/512v10t4g4 2,I1/64t32Zg32,G1/512v10t4g4 2,I1/64t32Zg32,G1/512v10t4g4 2,I1/64t32Zg32,G1/512v10t4g4 2,I1/128t32Zg32,G1/512v10t8g8 2,I16/4096t32Rg512,G1/512v10t256g256 2,I32/100032t32Rg1024,G1/512v10t6252g1024
pair ww sw0: 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/128t32Zg32,I1/128t32Zg32 F512,I16/4096t32Rg512,I16/4096t32Rg512 F1024,I32/100032t32Rg1024,I32/100032t32Rg1024
pair ww sw1: 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/128t32Zg32,I1/128t32Zg32 F512,I16/4096t32Rg512,I16/4096t32Rg512 F1024,I32/100032t32Rg1024,I32/100032t32Rg1024
pair ww ws 3M sw0: 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/128t32Zg32,I1/128t32Zg32 2,I16/4096t32Rg512,I16/4096t32Rg512 2,I1/100032t32Zg32,I32/100032t32Rg1024
pair ww ws 3M sw1: 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/128t32Zg32,I1/128t32Zg32 2,I16/4096t32Rg512,I16/4096t32Rg512 2,I1/100032t32Zg32,I32/100032t32Rg1024
pair ww shapes differ sw0: 2,I1/64t32Zg32,I1/64t16Zg16 2,I1/64t32Zg32,I1/64t16Zg16 2,I1/64t32Zg32,I1/64t16Zg16 2,I1/64t32Zg32,I1/64t16Zg16 2,I1/128t32Zg32,I1/128t16Zg16 2,I16/4096t32Rg512,I16/4096t16Rg256 2,I32/100032t32Rg1024,I64/100032t16Rg1024
pair ww shapes differ sw1: 2,I1/64t32Zg32,I1/64t16Zg16 2,I1/64t32Zg32,I1/64t16Zg16 2,I1/64t32Zg32,I1/64t16Zg16 2,I1/64t32Zg32,I1/64t16Zg16 2,I1/128t32Zg32,I1/128t16Zg16 2,I16/4096t32Rg512,I16/4096t16Rg256 2,I32/100032t32Rg1024,I64/100032t16Rg1024
pair ww ws misaligned sw0: 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/128t32Zg32,I1/128t32Zg32 2,I1/4096t32Zg32,I16/4096t32Rg512 2,I1/100032t32Zg32,I32/100032t32Rg1024
pair ww ws misaligned sw1: 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/64t32Zg32,I1/64t32Zg32 2,I1/128t32Zg32,I1/128t32Zg32 2,I1/4096t32Zg32,I16/4096t32Rg512 2,I1/100032t32Zg32,I32/100032t32Rg1024
pair ww b A misaligned sw0: 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/128t32Zg32,G1/128v01t32Zg32 2,I16/4096t32Rg512,G16/4096v01t32Rg512 2,I32/100032t32Rg1024,G32/100032v01t32Rg1024
pair ww b A misaligned sw1: 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/128t32Zg32,G1/128v01t32Zg32 2,I16/4096t32Rg512,G16/4096v01t32Rg512 2,I32/100032t32Rg1024,G32/100032v01t32Rg1024
pair ww b stored nn sw0: 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/128t32Zg32,G1/128v01t32Zg32 2,I16/4096t32Rg512,G16/4096v01t32Rg512 2,I32/100032t32Rg1024,G32/100032v01t32Rg1024
pair ww b stored nn sw1: 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/64t32Zg32,G1/64v01t32Zg32 2,I1/128t32Zg32,G1/128v01t32Zg32 2,I16/4096t32Rg512,G16/4096v01t32Rg512 2,I32/100032t32Rg1024,G32/100032v01t32Rg1024
pair ww guarded sw0: 2,G1/64t32Zg32,G1/64t32Zg32 2,G1/64t32Zg32,G1/64t32Zg32 2,G1/64t32Zg32,G1/64t32Zg32 2,G1/64t32Zg32,G1/64t32Zg32 2,G1/128t32Zg32,G1/128t32Zg32 2,G16/4096t32Rg512,G16/4096t32Rg512 2,G32/100032t32Rg1024,G32/100032t32Rg1024
pair ww guarded sw1: 2,G1/64t32Zg32,G1/64t32Zg32 2,G1/64t32Zg32,G1/64t32Zg32 2,G1/64t32Zg32,G1/64t32Zg32 2,G1/64t32Zg32,G1/64t32Zg32 2,G1/128t32Zg32,G1/128t32Zg32 2,G16/4096t32Rg512,G16/4096t32Rg512 2,G32/100032t32Rg1024,G32/100032t32Rg1024
pair xx sw0: F4,I1/512t4g4,I1/96t2g2 F4,I1/512t4g4,I1/96t2g2 F4,I1/512t4g4,I1/96t2g2 F4,I1/512t4g4,I1/96t2g2 F8,I1/512t8g8,I1/96t4g4 F256,I1/512t256g256,I1/96t128g128 F1024,I1/512t6252g1024,I1/96t3126g1024
pair xx sw1: F4,I1/512t4g4,I1/96t2g2 F4,I1/512t4g4,I1/96t2g2 F4,I1/512t4g4,I1/96t2g2 F4,I1/512t4g4,I1/96t2g2 F8,I1/512t8g8,I1/96t4g4 F256,I1/512t256g256,I1/96t128g128 F1024,I1/512t6252g1024,I1/96t3126g1024
pair xx b guarded sw0: 2,I1/512t4g4,G1/96t2g2 2,I1/512t4g4,G1/96t2g2 2,I1/512t4g4,G1/96t2g2 2,I1/512t4g4,G1/96t2g2 2,I1/512t8g8,G1/96t4g4 2,I1/512t256g256,G1/96t128g128 2,I1/512t6252g1024,G1/96t3126g1024
pair xx b guarded sw1: 2,I1/512t4g4,G1/96t2g2 2,I1/512t4g4,G1/96t2g2 2,I1/512t4g4,G1/96t2g2 2,I1/512t4g4,G1/96t2g2 2,I1/512t8g8,G1/96t4g4 2,I1/512t256g256,G1/96t128g128 2,I1/512t6252g1024,G1/96t3126g1024
pair xx a K guarded sw0: 2,G1/50v01t4g4,I1/96t2g2 2,G1/50v01t4g4,I1/96t2g2 2,G1/50v01t4g4,I1/96t2g2 2,G1/50v01t4g4,I1/96t2g2 2,G1/50v01t8g8,I1/96t4g4 2,G1/50v01t256g256,I1/96t128g128 2,G1/50v01t6252g1024,I1/96t3126g1024
pair xx a K guarded sw1: 2,G1/50v01t4g4,I1/96t2g2 2,G1/50v01t4g4,I1/96t2g2 2,G1/50v01t4g4,I1/96t2g2 2,G1/50v01t4g4,I1/96t2g2 2,G1/50v01t8g8,I1/96t4g4 2,G1/50v01t256g256,I1/96t128g128 2,G1/50v01t6252g1024,I1/96t3126g1024
pair xx a A misaligned sw0: 2,G1/512v01t4g4,I1/96t2g2 2,G1/512v01t4g4,I1/96t2g2 2,G1/512v01t4g4,I1/96t2g2 2,G1/512v01t4g4,I1/96t2g2 2,G1/512v01t8g8,I1/96t4g4 2,G1/512v01t256g256,I1/96t128g128 2,G1/512v01t6252g1024,I1/96t3126g1024
pair xx a A misaligned sw1: 2,G1/512v01t4g4,I1/96t2g2 2,G1/512v01t4g4,I1/96t2g2 2,G1/512v01t4g4,I1/96t2g2 2,G1/512v01t4g4,I1/96t2g2 2,G1/512v01t8g8,I1/96t4g4 2,G1/512v01t256g256,I1/96t128g128 2,G1/512v01t6252g1024,I1/96t3126g1024
pair xx b stored tn sw0: 2,I1/512t4g4,G1/96v01t2g2 2,I1/512t4g4,G1/96v01t2g2 2,I1/512t4g4,G1/96v01t2g2 2,I1/512t4g4,G1/96v01t2g2 2,I1/512t8g8,G1/96v01t4g4 2,I1/512t256g256,G1/96v01t128g128 2,I1/512t6252g1024,G1/96v01t3126g1024
pair xx b stored tn sw1: 2,I1/512t4g4,G1/96v01t2g2 2,I1/512t4g4,G1/96v01t2g2 2,I1/512t4g4,G1/96v01t2g2 2,I1/512t4g4,G1/96v01t2g2 2,I1/512t8g8,G1/96v01t4g4 2,I1/512t256g256,G1/96v01t128g128 2,I1/512t6252g1024,G1/96v01t3126g1024
pair xx b batched sw0: 2,I1/512t4g4,x 2,I1/512t4g4,x 2,I1/512t4g4,x 2,I1/512t4g4,x 2,I1/512t8g8,x 2,I1/512t256g256,x 2,I1/512t6252g1024,x
pair xx b batched sw1: 2,I1/512t4g4,x 2,I1/512t4g4,x 2,I1/512t4g4,x 2,I1/512t4g4,x 2,I1/512t8g8,x 2,I1/512t256g256,x 2,I1/512t6252g1024,x
"""


def test_gemm_plan_is_the_decision_the_scattered_predicates_made():
    """gcgcn_debug_gemm_plan (the plan function every launcher of gemm.hip calls) gives, for every row, the launch the code before it
    chose: interior or guarded, split factor, ksplit, widen, kept row-block mode, vector flags, tiles, reduce and zero-fill launches,
    grid, and for a pair fused or not and gridW.  No tolerance, no row left out."""
    import ctypes
    import numpy as np

    def plan(form, a, b, splits, group_work, cap):
        out = np.full(26, -7, np.int32)
        pa = (ctypes.c_int64 * 13)(*a)
        pb = (ctypes.c_int64 * 13)(*b) if b is not None else None
        _lib.call("gcgcn_debug_gemm_plan", form, pa, pb, splits, group_work, cap, out.ctypes.data_as(ctypes.c_void_p))
        return [int(v) for v in out]

    got, plans = gemm_plan_table(plan, lambda name, v: _lib.call("gcgcn_set_option", name.encode(), v))
    want = GEMM_PLAN_EXPECTED.strip("\n").split("\n")
    assert len(got) == len(want) == 2 * (3 * len(GEMM_PLAN_CASES) + len(GEMM_PAIR_CASES)) == 212
    assert plans == 2 * ((5 + 2 * len(GEMM_PLAN_CAPS)) * len(GEMM_PLAN_CASES) + len(GEMM_PLAN_CAPS) * len(GEMM_PAIR_CASES)) == 1372
    wrong = [f"want {w}\n got {g}" for g, w in zip(got, want) if g != w]
    assert not wrong, "\n".join(wrong[:20])
