"""What the producer's edge suite (producer_cases.py, test_producer_edges_gpu.py) rests on, checked without a GPU: the float64
folded oracle equals the unfolded one, the bound is not vacuous, the relu-flip cap holds, the cases reach what they were written
for (every distance id on both sides, every range length, junk that really is out of range, the 1e-10 case without a padded
slot).

The float32 oracle against the float64 oracle, worst fraction of the bound over all 69 cases: E 0.093, d ctx 0.030, d node 0.018,
d dis_table 0.023, parameter gradients 0.134 (d word_attention.attention_all.bias in the all-live case: the softmax is invariant
under that bias, so the reference is zero and the error is the rounding of cancelling terms against the bound's absolute floor;
at N = 64 / 91 the same tensor moves between 0.01 and 0.09 with the number of CPU threads);
every other parameter gradient at most 0.068.  test_float32_oracle_is_well_inside_the_bound keeps every case under 0.25; the
cases in producer_cases.SEEDS drew inputs at seed 0 that did not (a pair divided by 1e-10 whose largest sentence score is a few
1e-3: the float32 rounding of that score is 1e-5 of the whole row) or whose sentence scores all had one sign."""
import pytest
import torch

from oracle import gcgcn_oracle as O
import producer_cases as C

CASES = C.ALL_CASES
IDS = [f"{fam}:{C.kw_id(kw)}" for fam, kw in CASES]


def test_folded_oracle_equals_unfolded_in_float64():
    """test_oracle_golden.py pins both restatements to the reference's own classes in float32 (2e-5); here the two against each
    other in float64, forward and every gradient, 1e-12 relative -- with holes, junk-free ids and a pair divided by 1e-10."""
    c = C.make_case(B=1, N=3, S=2, T=7, Hd=4, P=3, ND=5, holes=True, seed=1)
    assert c.full.any()
    res = []
    for fn in (O.edge_features, O.edge_features_folded):
        sd = {f"{k.split('.', 1)[0]}.0.{k.split('.', 1)[1]}": v.double().requires_grad_() for k, v in c.sd.items()}
        leaves = [t.double().requires_grad_() for t in (c.ctx[0], c.node[0], c.table)]
        e = fn(leaves[0], c.sen[0], c.ph_ref[0], c.pt_ref[0], leaves[1], leaves[2], sd, 0)
        (e * (c.cot0[0].double() * torch.where(c.full[0], 1e-10, 1.0).unsqueeze(-1))).sum().backward()
        res.append([e.detach()] + [t.grad for t in leaves] + [v.grad for v in sd.values()])
    for a, b in zip(*res):
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("fam,kw", CASES, ids=IDS)
def test_float32_oracle_is_well_inside_the_bound(fam, kw):
    """A plain float32 evaluation of the same graph, with the same cotangent, uses under a quarter of the bound on every tensor:
    the inputs are well conditioned and the bound leaves a kernel no slack that float32 arithmetic does not need."""
    c, ref = C.case_and_ref(kw)
    res = C.ratios(C.reference(c, torch.float32, cot=ref["cot"]), ref)
    print(f"[prod-err] float32 oracle {fam} {c.id}: {C.short(res)}")
    assert max(res.values()) < 0.25, res


@pytest.mark.parametrize("fam,kw", CASES, ids=IDS)
def test_case_properties(fam, kw):
    c, ref = C.case_and_ref(kw)
    ND = c.ND
    # the relu-flip cap
    assert ref["flips"] <= C.FLIP_CAP, f"{ref['flips']:.3f} of the live pairs lie inside the flip margin: change the case's seed"
    # sentence scores of either sign (both branches of the relu), except where every live pair is divided by 1e-10
    sc = ref["scores"][c.live_slots]
    if c.scale_full:
        assert sc.numel() == 0 or (float(sc.min()) >= 0.5 and float(sc.max()) <= 2.5)
    elif c.mask in ("random", "token0") and c.rows >= 10:
        assert 0.15 <= float((sc > 0).float().mean()) <= 0.85
    # every distance id is used by a live, unmasked token of a real pair, on both sides -- wherever the case has ND such tokens
    assert c.covers or c.mask != "random" or fam in ("T", "N"), f"only {c.live_tokens} live tokens for {ND} ids"
    if c.covers:
        for k in (c.ph_ref, c.pt_ref):
            assert set(k[c.used].tolist()) == set(range(ND))
    # junk ids: out of range wherever the producer must not look; the kernel's copy equals the reference's on the rest
    for k, kref in ((c.ph, c.ph_ref), (c.pt, c.pt_ref)):
        k = k.long()
        assert torch.equal(k[c.used], kref[c.used]) and ((kref >= 0) & (kref < ND)).all() and (kref[~c.used] == 0).all()
        assert ((k[~c.used] < 0) | (k[~c.used] >= ND)).all()
    # the counts the GPU tests compare with
    assert c.rows == int((c.sen[..., 0] & c.pair.unsqueeze(-1)).sum()) and 0 <= c.pairs <= c.rows
    if c.ragged:
        pad = ~c.real
        assert (c.node[pad].abs() >= 500).all() and torch.isfinite(c.node).all()
        assert c.sen[~c.pair][..., 0].any(), "padding pairs hold live-looking slots"
        assert float(ref["d node"][pad].abs().sum()) == 0.0 and float(ref["E"][~c.pair].abs().sum()) == 0.0
    if c.mask == "all_live":
        assert c.full[c.pair].all() and c.scale_full and c.rows == c.pairs * c.S
        assert float(ref["cot"][c.pair].abs().max()) < 1e-9 and float(ref["E"].abs().max()) > 1e6
    if c.mask == "none_live":
        assert c.rows == 0
    if c.mask == "one_live":
        assert c.rows == 1 and c.pairs == 1
    if c.mask == "token0":
        assert (c.sen[c.live_slots].sum(-1) == 1).all() and c.rows > 0


def test_what_the_sweeps_reach():
    """The properties single sweeps were written for."""
    live_len = lambda c: set(c.sen[c.live_slots].sum(-1).tolist())
    c = C.make_case()
    assert {1, 2, 3, 4, 5, 7, 8} <= live_len(c) and c.covers
    for kw in C.SWEEPS["ND"] + C.SWEEPS["Hd"] + C.SWEEPS["Hd x ND"] + C.SWEEPS["ragged"] + C.SWEEPS["dtype"] + C.SWEEPS["P"]:
        assert C.make_case(**kw).covers, kw
    c = C.make_case(T=2048, N=3)
    ends = c.sen[c.live_slots].float().cumsum(-1).argmax(-1) + 1                   # one past the last token of each live slot
    assert 2048 in ends.tolist() and any(512 < e < 2048 for e in ends.tolist())
    dead = c.sen[~c.live_slots & c.pair.unsqueeze(-1)]
    assert (dead[:, 510] & dead[:, 513]).any() and dead[:, -1].any() and not dead[:, 0].any()
    c = C.make_case(holes=True)
    rng = c.sen[c.live_slots]
    assert any((r.nonzero().max() + 1 > r.sum()).item() for r in rng), "no live slot has a hole"
    n = C.make_case(N=46, S=1, T=8)
    assert n.N * n.N > 2048                                                          # second trip of index pass A
    n = C.make_case(N=64, S=1, T=8)
    assert 2 * n.rows > 2048 * 4                                                     # more (row, side) items than row waves
    n = C.make_case(N=91, S=1, T=8, live=1.0)
    assert n.pairs > 2048 * 4                                                        # more live pairs than pair waves
    for kw in C.SWEEPS["N"] + C.SWEEPS["S"][:1]:
        c = C.make_case(**kw)
        assert c.scale_full == (c.S == 1) and (c.S > 1 or c.full[c.live_slots.any(-1)].all())
