"""The GEMM layer's suite without a GPU: the float64 restatement of gemm_layer_cases.py against a plain triple loop in Python floats
on one tiny case per feature, every case table through gcgcn_debug_gemm_plan (a case that no longer reaches its route fails here,
before it reaches a GPU), the restatement's own windows on every case, and the argument list of gcgcn_debug_gemm_run against the
layout include/gcgcn.h documents."""
import ctypes
import re

import pytest
import torch

import gemm_layer_cases as G
from gcgcn_amd import _lib

CASES = G.all_cases()
FLOAT64_SLACK = 2.0 ** -40      # two float64 summation orders of a few dozen terms of order one


def loop_reference(q, T, keep):
    """csrc/gemm.hpp's epilogue, element by element in Python floats -> {(buffer, index): value}"""
    buf = lambda name: T[q.ptr[name][0]].tolist()
    A, B, C = buf("A"), buf("B"), buf("C")
    opt = {name: buf(name) for name in ("add", "bias", "rowadd", "rowscale", "add2") if name in q.ptr}
    nv = T[q.ptr["n_valid"][0]].tolist() if "n_valid" in q.ptr else None
    lst = T[q.ptr["rb"][0]].tolist() if q.rb_mode else None
    live = set(lst[4:4 + lst[0]]) if lst else None
    out = {}
    for z1 in range(q.batch1):
        for z2 in range(q.batch2):
            for row in range(q.M):
                dead = q.rb_mode == 1 and row // 16 not in live
                if dead and not q.rb_zero:
                    continue
                for col in range(q.N):
                    acc = 0.0
                    for k in range(q.K):
                        if q.rb_mode == 2 and k // 16 not in live:
                            continue
                        a = A[q.ptr["A"][1] + z1 * q.sA1 + z2 * q.sA2 + (row * q.lda + k if q.a_kc else k * q.lda + row)]
                        b = B[q.ptr["B"][1] + z1 * q.sB1 + z2 * q.sB2 + (col * q.ldb + k if q.b_kc else k * q.ldb + col)]
                        acc += a * b
                    v = q.alpha * acc
                    if "add" in opt:
                        v += opt["add"][q.ptr["add"][1] + z1 * q.sAdd1 + z2 * q.sAdd2 + row * q.ldadd + col]
                    if "bias" in opt:
                        v += opt["bias"][q.ptr["bias"][1] + col]
                    if "rowadd" in opt:
                        v += opt["rowadd"][q.ptr["rowadd"][1] + z1 * q.sRa1 + z2 * q.sRa2 + row]
                    if "rowscale" in opt:
                        v *= opt["rowscale"][q.ptr["rowscale"][1] + z1 * q.sRs1 + z2 * q.sRs2 + row]
                    if q.relu:
                        v = max(v, 0.0)
                    oc = q.ptr["C"][1] + z1 * q.sC1 + z2 * q.sC2 + row * q.ldc + col
                    if q.accumulate:
                        v += C[oc]
                    pad = dead or (nv is not None and row % q.nv_rows >= nv[z1 * q.nv_zdoc + row // q.nv_rows])
                    if pad:
                        v = 0.0
                    out[(q.ptr["C"][0], oc)] = v
                    if "C2" in q.ptr:
                        o2 = z1 * q.sC21 + z2 * q.sC22 + row * q.ldc2 + col
                        w = v
                        if q.p > 0:
                            w = w / (1.0 - q.p) if keep[q.drop_base + o2] else 0.0
                        if "add2" in opt:
                            w += opt["add2"][q.ptr["add2"][1] + z1 * q.sAdd21 + z2 * q.sAdd22 + row * q.ldadd2 + col]
                        out[(q.ptr["C2"][0], q.ptr["C2"][1] + o2)] = 0.0 if pad else w
    return out


def fake_keep(q, seed):
    return (torch.rand(G.keep_extent(q), generator=torch.Generator().manual_seed(seed)) >= q.p).to(torch.uint8)


def tiny_cases():
    cases = []
    for feat in G.FEATURE_SETS:
        for form in G.FORMS:
            b = G.Builder(f"tiny-{form}-{feat}", G.FORM_GEMM, 40 + len(cases))
            b.problem(form, 5, 3, 4, G.FEATURE_SETS[feat], relu=len(cases) % 2, accumulate=(len(cases) // 2) % 2, batch=(2, 2),
                      p=0.25 if "C2" in G.FEATURE_SETS[feat] else 0.0)
            cases.append(b.case)
    b = G.Builder("tiny-n_valid", G.FORM_GEMM, 90)
    b.problem("nn", 8, 3, 4, G.ALL_FEATS, 1, 1, batch=(2, 2), p=0.25, n_valid=[0, 1, 4, 2, 3], nv_rows=4, nv_zdoc=1)
    cases.append(b.case)
    for rb_zero in (0, 1):
        b = G.Builder(f"tiny-rb1-z{rb_zero}", G.FORM_GROUP, 91 + rb_zero)
        b.case.ints["rb"] = G.live_blocks([17, 0, 1], 32)
        b.problem("nn", 96, 3, 4, G.ALL_FEATS, 1, 1, p=0.25, rb="rb", rb_mode=1, rb_zero=rb_zero, n_valid=[17, 0, 1], nv_rows=32)
        cases.append(b.case)
    b = G.Builder("tiny-rb2", G.FORM_GEMM, 93)
    b.case.ints["rb"] = G.live_blocks([17, 0, 1], 32)
    b.problem("tn", 3, 5, 96, ("alpha",), 0, 1, rb="rb", rb_mode=2)
    cases.append(b.case)
    cases += [G.stack_case(k, N=4, gh=3, L=2, H=2, B=2) for k in ("dense", "agg", "dP", "dA", "dY")]
    return cases


TINY = tiny_cases()


@pytest.mark.parametrize("case", TINY, ids=[c.name for c in TINY])
def test_restatement_equals_a_triple_loop(case):
    T = G.tensors_of(case)
    keeps = {i: fake_keep(q, 7 + i) for i, q in enumerate(case.probs) if q.p > 0}
    ref = G.reference(case, T, keeps)
    want = {}
    for i, q in enumerate(case.probs):
        want.update(loop_reference(q, T, keeps.get(i)))
    assert want, case.name
    seen = {name: 0 for name in ref}
    for (name, idx), v in want.items():
        exp, bound, written = ref[name]
        assert written[idx], f"{name}[{idx}] is written by the loop, not by the restatement"
        assert abs(float(exp[idx]) - v) <= FLOAT64_SLACK * (1.0 + abs(v)), f"{name}[{idx}]: {float(exp[idx])} against {v}"
        seen[name] += 1
    for name, (exp, bound, written) in ref.items():
        assert int(written.sum()) == seen[name], f"{name}: the restatement writes elements the loop does not"


def test_live_blocks_is_the_documented_list():
    assert G.live_blocks([0, 17, 64], 64) == [6, 0, 0, 0, 4, 5, 8, 9, 10, 11, 0, 1, 2, 3, 6, 7]
    assert G.live_blocks([0, 0], 32) == [0, 0, 0, 0, 0, 1, 2, 3]


@pytest.mark.parametrize("group", list(G.GROUPS))
def test_every_case_takes_the_route_it_means(group):
    cases = [c for g, c in CASES if g == group]
    assert cases
    for case in cases:
        plans = G.assert_routes(case, _lib.call)
        assert any(case.expect) and len(plans) == len(case.probs) or not case.probs, case.name
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)


def test_the_tables_hold_what_the_suite_is_about():
    by = {g: [c for gg, c in CASES if gg == g] for g in G.GROUPS}
    interior = lambda c: [e.get("interior") for e in c.expect]
    assert {1, 0} <= {i for c in by["epilogue"] for i in interior(c)}
    assert {tuple(c.ints["rb"][:1]) for c in by["rb1"]} >= {(6,), (12,), (6,), (0,)}
    assert {e.get("widen") for c in by["rb1"] for e in c.expect} >= {1, 2, 4}
    assert {len(c.probs) for c in by["group"]} >= {2, 9, 11} and max(len(c.probs) for c in by["group"]) > G.MAXP
    assert {c.ride.kind for c in by["ride"]} == {1, 2, 3} and any(c.ride.later_expected for c in by["ride"])
    assert any(0 in c.accepted[2:] for c in by["park"]) and all(c.accepted[1] == 0 for c in by["park"])
    assert {e.get("fused") for c in by["pairs"] for e in c.expect} == {0, 1}
    assert {c.form for c in by["pairs"]} == {G.FORM_PAIR_WX, G.FORM_PAIR_WW, G.FORM_PAIR_XX}
    assert {c.cnt for c in by["pairs"]} >= {0, 1, 63, 64, 65, 200}


@pytest.mark.parametrize("group", list(G.GROUPS))
def test_restatement_windows_of_every_case(group):
    """reference() on every case: no two problems write one element, every window lies inside its buffer with the margin in front and
    the slack behind untouched, every bound is finite and not negative."""
    for case in (c for g, c in CASES if g == group):
        T = G.tensors_of(case)
        keeps = {i: fake_keep(q, i) for i, q in enumerate(case.probs) if q.p > 0}
        interior = {i: bool(getattr(case, "interior", False)) for i in range(len(case.probs))}
        for name, (exp, bound, written) in G.reference(case, T, keeps, interior).items():
            assert case.buffers[name][1] == "out", f"{case.name}: {name} is written but is no output buffer"
            assert not written[:4].any() and not written[-8:].any(), f"{case.name}: {name} has no margin left"
            assert torch.isfinite(exp[written]).all() and torch.isfinite(bound).all() and (bound >= 0).all(), f"{case.name}: {name}"


def test_argument_list_is_the_documented_layout():
    res, args = _lib.SIGNATURES["gcgcn_debug_gemm_run"]
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert res is I and args == [I, I, P, P, P, P, P, I, I, P, L, P, P]
    assert len(G.INT_ORDER) == G.NI == 40 and len(G.PTR_ORDER) == G.NP == 14 and G.NF == 2
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    doc = header[header.index("run what the GEMM launcher launches"):header.index("int gcgcn_debug_gemm_run")]
    flat = " ".join(doc.replace("*", " ").split())
    assert "int64[40]" in flat and "float[2]" in flat and "14 device pointers" in flat and "int32[2 + 2 n]" in flat
    at = [flat.index(name) for name in ("sA1, sA2, sB1, sB2, sC1, sC2", "ldadd, sAdd1, sAdd2", "sRa1, sRa2, sRs1, sRs2", "ldc2, sC21, sC22",
                                        "ldadd2, sAdd21, sAdd22", "relu", "accumulate", "nv_rows", "nv_zdoc", "rb_zero", "drop_base", "salt")]
    assert at == sorted(at)
    assert re.search(r"A, B, C, add, bias, rowadd, rowscale, C2, add2, n_valid, rb, rb_n, ws, rng_snap", flat)
    plan_doc = " ".join(header[header.index("what the GEMM launcher decides"):header.index("int gcgcn_debug_gemm_plan")].replace("*", " ").split())
    assert "M, N, K, a_kc, b_kc, lda, ldb, ldc, batch1, batch2, row-block mode, workspace elements" in plan_doc
    assert list(G.INT_ORDER[:12]) == ["M", "N", "K", "a_kc", "b_kc", "lda", "ldb", "ldc", "batch1", "batch2", "rb_mode", "ws_elems"]
    case = G.epilogue_case("nn", "i64", "all", 1, 1, p=0.25)
    ints, scal, ptrs, ride, rptr = G.pack(case, lambda name: 1 << 20)
    assert ints.shape == (1, 40) and scal.shape == (1, 2) and ptrs.shape == (1, 14) and ride.shape == (6,) and rptr.shape == (3,)
    q = case.probs[0]
    assert list(ints[0, :13]) == [64, 64, 32, 1, 0, q.lda, q.ldb, q.ldc, 1, 1, 0, 0, 0] and ints[0, 37] == q.drop_base and ints[0, 38] == q.salt
    assert (ptrs[0, [9, 10, 11, 12]] == 0).all() and (ptrs[0, [0, 1, 2, 3, 4, 5, 6, 7, 8, 13]] != 0).all()
