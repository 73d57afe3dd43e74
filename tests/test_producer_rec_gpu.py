"""The record route of the edge-feature producer on the GPU (csrc/producer_rec.hip, functional.edge_features(slot_records=...)).

The dense tensors are built by the unchanged data.collate and the reference is the unchanged dense route, never the code under test:
on the hand-made batches of producer_rec_cases the two routes must agree bit for bit -- E, the compact rows and the pair index, every
gradient of the deterministic backward, the device-side counts -- whatever the order of the records.  The default (atomic) backward of
both routes is held against float64 autograd of the oracle's producer at the bound of the existing edge suite (producer_cases.ratios:
|got - ref| <= 1e-5 max(1, max|ref|) + 1e-4 |ref|), and the routes against each other at the same bound.  Then the host-side counts of
collate(dense_slots=False), the loud failure on capacities one too small, and a GraphedTrainStep over GraphModelTail fed by records
alone (no capacity computed by the caller), replayed on new records.  Last, the model level: GCGCN_glove (HIP encoder and front end,
deterministic) called, evaluated (evaluate) and trained (train_epoch) on a records batch gives bit for bit what the dense batch gives,
and GraphedTrainStep captures the whole model from a records batch."""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import data as D, functional as F_, models as M, params as P_
from gcgcn_amd.evaluation import forward_args
from gcgcn_amd.optim import FusedAdam, GraphedTrainStep
import producer_cases as PC
import producer_rec_cases as C

pytestmark = pytest.mark.gpu

GRADS = ("dctx", "dnode", "dtable", "dflat")
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _batch(name, shuffle=False):
    """(dense dict of the unchanged collate, record dict of collate(dense_slots=False), docs, (B, N, S, T))."""
    docs, N, S, T = C.BATCHES[name]()
    dense = D.collate(docs, DEV)
    assert tuple(dense["sen_matrix"].shape) == (len(docs), N, N, S, T)
    if shuffle:
        rng = np.random.default_rng(11)
        docs = copy.deepcopy(docs)
        for d in docs:
            d.slots = d.slots[rng.permutation(d.slots.shape[0])]
    rec = D.collate(docs, DEV, dense_slots=False)
    if shuffle:                                             # across the documents too
        perm = torch.from_numpy(np.random.default_rng(12).permutation(rec["slot_records"].shape[0])).to(DEV)
        rec["slot_records"] = rec["slot_records"][perm].contiguous()
    return dense, rec, docs, (len(docs), N, S, T)


def _inputs(shape, Hd, P=20, seed=0):
    B, N, S, T = shape
    g = torch.Generator().manual_seed(1000 + seed + Hd)
    ctx = torch.tanh(torch.randn(B, T, Hd, generator=g))
    node = torch.rand(B, N, Hd, generator=g) * 2 - 1
    table = torch.randn(21, P, generator=g) * 0.5
    cot = torch.randn(B, N, N, Hd, generator=g)
    return ctx, node, table, cot


def _producer(Hd, P, seed=0):
    torch.manual_seed(seed)
    return gcgcn_amd.EdgeFeatureProducer(Hd, P).to(DEV)


def _run(prod, inp, batch, route, det=True, compact=False, caps=None, check_capacity=None):
    dense, rec, _, _ = batch
    ctx, node, table, cot = inp
    prod.zero_grad()
    cg, ng, tg = (t.to(DEV).requires_grad_() for t in (ctx, node, table))
    kw = dict(n_valid=dense["n_valid"], compact=compact, deterministic=det, check_capacity=check_capacity)
    if caps is not None:
        kw.update(max_live_slots=caps[0], max_live_pairs=caps[1])
    if route == "dense":
        e = prod(cg, dense["sen_matrix"], dense["pos_matrix_h"], dense["pos_matrix_t"], ng, tg, **kw)
    else:
        e = prod(cg, None, None, None, ng, tg, slot_records=rec["slot_records"], slot_shape=rec["S"], **kw)
    out = {}
    if compact:
        rows = int(prod.last_counts[1])
        out["Ec"], out["prow"] = e.Ec.detach()[:rows].clone(), e.prow.clone()
        e = e.dense()
    (e * cot.to(DEV)).sum().backward()
    out.update(E=e.detach(), dctx=cg.grad, dnode=ng.grad, dtable=tg.grad, dflat=prod.flat.grad.clone(), counts=prod.last_counts.tolist())
    return out


def _assert_bitwise(a, b, what):
    assert a["counts"] == b["counts"], f"{what}: counts {a['counts']} != {b['counts']}"
    for k in [k for k in ("Ec", "prow") if k in a] + ["E"] + list(GRADS):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), \
            f"{what}: {k} differs (max |diff| {(a[k].float() - b[k].float()).abs().max().item():.3e})"


# the two shapes of the contract at the reference's width, and the first at the smallest width of the existing producer suites (Hd = 1:
# one column, no float4 path in prod_word_bwd_rows) and at a ragged one (24)
CASES = [("hand", 128), ("t1", 128), ("hand", 1), ("hand", 24)]


@pytest.mark.parametrize("compact", [False, True], ids=["dense-E", "compact"])
@pytest.mark.parametrize("name,Hd", CASES, ids=[f"{n}-Hd{h}" for n, h in CASES])
def test_record_route_equals_dense_route_bitwise(gpu_device, name, Hd, compact):
    batch = _batch(name)
    P = 20 if Hd > 1 else 3
    inp, prod = _inputs(batch[3], Hd, P), _producer(Hd, P)
    want = _run(prod, inp, batch, "dense", compact=compact)
    got = _run(prod, inp, batch, "rec", compact=compact)
    assert want["counts"][0] > 0 and want["counts"][2] == 0 and torch.isfinite(want["E"]).all()
    assert all(torch.isfinite(want[k]).all() for k in GRADS) and want["dflat"].abs().sum() > 0
    _assert_bitwise(got, want, "records / dense")
    again = _run(prod, inp, batch, "rec", compact=compact)
    _assert_bitwise(again, got, "records, second run")
    shuffled = _run(prod, inp, _batch(name, True), "rec", compact=compact)
    _assert_bitwise(shuffled, want, "shuffled records / dense")
    # with the host-side capacities of collate(dense_slots=False): exactly enough
    rec = batch[1]
    exact = _run(prod, inp, batch, "rec", compact=compact, caps=(rec["max_live_slots"], max(rec["max_live_pairs"], 1)))
    assert exact["counts"][:3] == want["counts"][:3]
    for k in ("E",) + GRADS:
        assert torch.equal(exact[k], want[k]), k


@pytest.mark.parametrize("compact", [False, True], ids=["dense-E", "compact"])
def test_a_batch_without_live_slots(gpu_device, compact):
    batch = _batch("none_live")
    inp, prod = _inputs(batch[3], 128), _producer(128, 20)
    want = _run(prod, inp, batch, "dense", compact=compact)
    got = _run(prod, inp, batch, "rec", compact=compact)
    assert want["counts"][:3] == [0, 0, 0]
    _assert_bitwise(got, want, "records / dense, no live slot")
    bias = prod.named_tensors()["linear_sentence_att.bias"]
    nv = batch[0]["n_valid"]
    for b in range(batch[3][0]):
        n = int(nv[b])
        assert torch.equal(got["E"][b, :n, :n], bias.expand(n, n, -1)) and not got["E"][b, n:].any() and not got["E"][b, :, n:].any()


def test_collate_without_dense_slots(gpu_device):
    """Every other key of the dict is what the default returns; the three tensors are gone; the counts are the dense route's."""
    for name in C.BATCHES:
        dense, rec, docs, (B, N, S, T) = _batch(name)
        assert set(dense) - set(rec) == {"sen_matrix", "pos_matrix_h", "pos_matrix_t"}
        assert set(rec) - set(dense) == {"slot_records", "S", "max_live_slots", "max_live_pairs"}
        for k in set(dense) & set(rec) - {"_keep"}:
            assert torch.equal(dense[k], rec[k]), k
        assert rec["S"] == S and rec["slot_records"].dtype == torch.int32 and rec["slot_records"].shape[1] == 10
        assert isinstance(rec["max_live_slots"], int) and isinstance(rec["max_live_pairs"], int)
        assert (rec["max_live_slots"], rec["max_live_pairs"]) == F_.producer_live_counts(dense["sen_matrix"].view(torch.uint8), dense["n_valid"])
        sen, ph, pt = C.dense_numpy(docs, N, S, T)           # the restatement the CPU test counts on is what the kernel writes
        assert np.array_equal(dense["sen_matrix"].cpu().numpy(), sen != 0)
        assert np.array_equal(dense["pos_matrix_h"].cpu().numpy(), ph) and np.array_equal(dense["pos_matrix_t"].cpu().numpy(), pt)


def test_capacities_one_too_small_fail_loudly(gpu_device):
    batch = _batch("hand")
    dense, rec, _, (B, N, S, T) = batch
    inp, prod = _inputs(batch[3], 128), _producer(128, 20)
    r, q = rec["max_live_slots"], rec["max_live_pairs"]
    ctx, node, table, _ = (t.to(DEV) for t in inp)
    nv = dense["n_valid"]
    for caps in ((r - 1, q), (r, q - 1), (r - 1, q - 1)):
        kw = dict(n_valid=nv, slot_records=rec["slot_records"], slot_shape=S, max_live_slots=caps[0], max_live_pairs=caps[1])
        e = prod(ctx, None, None, None, node, table, **kw)
        assert prod.last_counts.tolist()[2] == 1
        for b in range(B):
            n = int(nv[b])
            assert torch.isnan(e[b, :n, :n]).all() and (e[b, n:] == 0).all() and (e[b, :, n:] == 0).all()
        ec = prod(ctx, None, None, None, node, table, compact=True, **kw)
        assert torch.isnan(ec.dense()[0, :int(nv[0]), :int(nv[0])]).all()
        with pytest.raises(F_.ProducerCapacityError, match="max_live_slots"):
            prod(ctx, None, None, None, node, table, check_capacity=True, **kw)
    e = prod(ctx, None, None, None, node, table, n_valid=nv, slot_records=rec["slot_records"], slot_shape=S, max_live_slots=r,
             max_live_pairs=q, check_capacity=True)
    assert prod.last_counts.tolist()[:3] == [r, q, 0] and torch.isfinite(e).all()


# ---- the default backward against float64 ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _f64_case(name, Hd, P):
    """The batch as a producer_cases case (its reference() and ratios() are the existing suite's) from the DENSE tensors."""
    dense, rec, docs, (B, N, S, T) = _batch(name)
    g = torch.Generator().manual_seed(77 + Hd)
    c = SimpleNamespace(B=B, N=N, S=S, T=T, Hd=Hd, P=P, ND=21, ns=[d.n for d in docs])
    c.ctx, c.node, c.table, _ = _inputs((B, N, S, T), Hd, P, seed=5)
    u = lambda shp, k: (torch.rand(*shp, generator=g) * 2 - 1) / k ** 0.5
    shapes = P_.producer_shapes(Hd, P)
    c.sd = {k: u(shp, shapes[k[:k.rindex(".")] + ".weight"][1]) for k, shp in shapes.items()}
    c.sd["sentence_attention.attention_all.weight"] *= 3.0
    c.sd["sentence_attention.attention_all.bias"] *= 0.1
    c.sen = dense["sen_matrix"].cpu()
    c.ph_ref, c.pt_ref = dense["pos_matrix_h"].cpu().long(), dense["pos_matrix_t"].cpu().long()
    real = torch.arange(N)[None, :] < torch.tensor(c.ns)[:, None]
    pair = real[:, :, None] & real[:, None, :]
    c.live_slots = c.sen[..., 0] & pair.unsqueeze(-1)
    c.pairs = int(c.live_slots.any(-1).sum())
    c.full, c.scale_full = pair & c.live_slots.all(-1), False
    c.node = c.node * real.unsqueeze(-1).float()
    c.cot0 = torch.randn(B, N, N, Hd, generator=g)
    return c, PC.reference(c)


def _run_case(c, ref, batch, route):
    dense, rec, _, _ = batch
    prod = gcgcn_amd.EdgeFeatureProducer(c.Hd, c.P)
    prod.load_state_dict(c.sd, strict=True)
    prod = prod.to(DEV)
    ctx, node, table = (t.to(DEV).requires_grad_() for t in (c.ctx, c.node, c.table))
    if route == "dense":
        e = prod(ctx, dense["sen_matrix"], dense["pos_matrix_h"], dense["pos_matrix_t"], node, table, n_valid=dense["n_valid"])
    else:
        e = prod(ctx, None, None, None, node, table, n_valid=dense["n_valid"], slot_records=rec["slot_records"], slot_shape=rec["S"])
    e.backward(ref["cot"].to(DEV))
    got = {"E": e.detach(), "d ctx": ctx.grad, "d node": node.grad, "d dis_table": table.grad}
    got.update({"d " + k: v for k, v in P_.unpack_producer(prod.flat.grad, c.Hd, c.P).items()})
    return got


@pytest.mark.parametrize("name,Hd", [("hand", 128), ("hand", 24)], ids=["hand-Hd128", "hand-Hd24"])
def test_default_backward_against_float64(gpu_device, name, Hd):
    c, ref = _f64_case(name, Hd, 20)
    assert not c.full.any()                                 # no pair of "hand" is divided by 1e-10 (producer_rec_cases)
    got = {route: _run_case(c, ref, _batch(name), route) for route in ("dense", "rec")}
    for route in ("dense", "rec"):
        res = PC.ratios(got[route], ref)
        print(f"[prod-rec-err] {name} Hd={Hd} {route}: {PC.short(res)}")
        bad = [f"{k}: {v:.3g} x bound" for k, v in res.items() if not v <= 1.0]
        assert not bad, f"{route} / float64: " + "; ".join(bad)
    res = PC.ratios(got["rec"], {k: v.cpu() for k, v in got["dense"].items()})
    print(f"[prod-rec-err] {name} Hd={Hd} rec / dense: {PC.short(res)}")
    bad = [f"{k}: {v:.3g} x bound" for k, v in res.items() if not v <= 1.0]
    assert not bad, "records / dense, default backward: " + "; ".join(bad)
    assert torch.equal(got["rec"]["E"], got["dense"]["E"])


# ---- the whole step, captured ---------------------------------------------------------------------------------------------------
def test_graphed_train_step_over_the_tail_from_records(gpu_device):
    """GraphedTrainStep over GraphModelTail (deterministic), fed by a collate(dense_slots=False) batch: no dense slot tensor, and no
    capacity computed by the caller -- nothing in the step reads the host.  It captures; two replays on NEW records of the same shapes
    equal two eager steps of a twin bit for bit (losses and every parameter)."""
    dev = gpu_device
    _, rec, docs, (B, N, S, T) = _batch("hand")
    docs2 = copy.deepcopy(docs)
    for d in docs2:                                         # other ranges and mention bounds, the same number of records
        d.slots[:, 4] += 3
        d.slots[:, 5:] += 2
    rec2 = D.collate(docs2, dev, dense_slots=False)
    assert rec2["slot_records"].shape == rec["slot_records"].shape and not torch.equal(rec2["slot_records"], rec["slot_records"])
    tables = [rec["slot_records"], rec2["slot_records"], rec["slot_records"].flip(0).contiguous()]
    g = torch.Generator().manual_seed(9)
    ctx, node, table, _ = _inputs((B, N, S, T), 128, 20, seed=3)
    nv = rec["n_valid"]
    ctx, table = ctx.to(dev).requires_grad_(), table.to(dev).requires_grad_()
    node = (node.to(dev) * (torch.arange(N, device=dev)[None, :] < nv[:, None]).unsqueeze(-1).float()).requires_grad_()
    ner = (torch.randn(7, 20, generator=g) * 0.3).to(dev).requires_grad_()
    ntype = torch.randint(0, 7, (B, N), generator=g).to(dev)
    rel = torch.randint(-10, 11, (B, N, N), generator=g).to(dev)
    labels = (torch.rand(B, N, N, 97, generator=g) < 0.05).float().to(dev)
    tail_g = gcgcn_amd.GraphModelTail().to(dev).eval()
    tail_e = gcgcn_amd.GraphModelTail().to(dev).eval()
    tail_g.deterministic = tail_e.deterministic = True
    tail_e.load_state_dict(tail_g.state_dict())

    def step_of(tail):
        def step_fn(label_matrix, n_valid, **kw):
            logits = tail(n_valid=n_valid, **kw)
            return gcgcn_amd.pair_bce_loss(logits, label_matrix, n_valid=n_valid).sum() / B
        return step_fn

    inputs = dict(context_output=ctx, node_feat=node, adj_matrix=None, sen_matrix=None, pos_matrix_h=None, pos_matrix_t=None,
                  node_type=ntype, node_relative_pos=rel, dis_embed_weight=table, ner_emb_weight=ner, n_valid=nv,
                  slot_records=tables[0].clone(), slot_shape=S, label_matrix=labels)
    params_g = [p for p in tail_g.parameters() if p.requires_grad]
    params_e = [p for p in tail_e.parameters() if p.requires_grad]
    og, oe = FusedAdam(params_g, lr=1e-4, capturable=True), FusedAdam(params_e, lr=1e-4, capturable=True)
    train = GraphedTrainStep(step_of(tail_g), og, inputs, warmup=2)
    step_e = step_of(tail_e)
    for k in (1, 2):
        loss_g = train(slot_records=tables[k])
        for p in params_e:
            p.grad = None
        loss_e = step_e(**dict(inputs, slot_records=tables[k]))
        loss_e.backward()
        oe.step()
        assert torch.isfinite(loss_g).all() and torch.equal(loss_g.detach(), loss_e.detach()), f"step {k}: {loss_g.item()} != {loss_e.item()}"
    torch.cuda.synchronize()
    moved = 0
    for (name, a), b_ in zip(tail_g.state_dict().items(), tail_e.state_dict().values()):
        assert torch.equal(a, b_), f"{name} differs after two steps"
    for p in params_g:
        moved += int(og.state.get(p) is not None and bool(og.state[p]["exp_avg"].any()))
    assert moved >= 4


# ---- the models, evaluate, train_epoch ---------------------------------------------------------------------------------------------
def _model_batches():
    docs, N, S, T = C.hand(n_rel=97)
    return D.collate(docs, DEV), D.collate(docs, DEV, dense_slots=False), len(docs)


def _glove(seed=21):
    """GCGCN_glove at the configuration of the model_step_c1 fixture (lstm_cases.Cfg), HIP encoder and front end, deterministic."""
    from lstm_cases import Cfg
    cfg = Cfg(30, "hip")
    cfg.frontend_impl, cfg.deterministic = "hip", True
    torch.manual_seed(seed)
    return M.GCGCN_glove(cfg).to(DEV)


def test_models_evaluate_and_train_epoch_on_a_records_batch(gpu_device):
    dense, rec, B = _model_batches()
    args_d, kw_d = forward_args(dense)
    args_r, kw_r = forward_args(rec)
    assert kw_d == {} and all(a is not None for a in args_d)
    assert [i for i, a in enumerate(args_r) if a is None] == [4, 5, 6]
    assert set(kw_r) == {"slot_records", "slot_shape", "max_live_slots", "max_live_pairs"} and kw_r["slot_shape"] == rec["S"]
    model = _glove().eval()
    with torch.no_grad():
        want = model(*args_d, n_valid=dense["n_valid"], t_valid=dense["t_valid"])
        got = model(*args_r, n_valid=rec["n_valid"], t_valid=rec["t_valid"], **kw_r)
    assert torch.isfinite(want).all() and torch.equal(got, want), "logits of the records batch differ from the dense batch's"
    ev_d, ev_r = gcgcn_amd.evaluate(model, [dense]), gcgcn_amd.evaluate(model, [rec])
    assert ev_d.n_records == ev_r.n_records > 0 and (ev_d.f1, ev_d.auc, ev_d.theta) == (ev_r.f1, ev_r.auc, ev_r.theta)
    assert torch.equal(ev_d.pr_y, ev_r.pr_y) and torch.equal(ev_d.pr_x, ev_r.pr_x)
    runs = []
    for bt in (dense, rec):
        m = _glove()
        opt = FusedAdam([p for p in m.parameters() if p.requires_grad], lr=1e-4)
        torch.manual_seed(12)
        gcgcn_amd.manual_seed(13)
        res = gcgcn_amd.train_epoch(m, opt, [bt, bt])
        runs.append((res, {k: v.clone() for k, v in m.state_dict().items()}))
    (res_d, sd_d), (res_r, sd_r) = runs
    assert res_d.n_steps == res_r.n_steps == 2 and np.isfinite(res_d.loss_sum) and res_d.loss_sum == res_r.loss_sum
    assert res_d.stats == res_r.stats
    start = _glove().state_dict()
    assert any(not torch.equal(sd_d[k], start[k]) for k in sd_d), "train_epoch did not train"
    for k in sd_d:
        assert torch.equal(sd_d[k], sd_r[k]), f"{k} differs after two steps of train_epoch"


def test_graphed_train_step_over_the_whole_model_from_records(gpu_device):
    """The capture DESIGN 8.7 records as refused by producer_live_counts' host read: GraphedTrainStep over GCGCN_glove with
    encoder_impl = frontend_impl = "hip", called as train_epoch calls the model, on a collate(dense_slots=False) batch.  It captures;
    replays on new records equal eager steps of a twin bit for bit."""
    dev = gpu_device
    _, rec, B = _model_batches()
    docs2, _, _, _ = C.hand(n_rel=97)
    for d in docs2:
        d.slots[:, 5:] += 2                                  # other mention bounds, the same ranges: the host-side capacities hold
    rec2 = D.collate(docs2, dev, dense_slots=False)
    assert rec2["slot_records"].shape == rec["slot_records"].shape and not torch.equal(rec2["slot_records"], rec["slot_records"])
    assert (rec2["max_live_slots"], rec2["max_live_pairs"]) == (rec["max_live_slots"], rec["max_live_pairs"])
    model_g, model_e = _glove().eval(), _glove().eval()
    args, kw = forward_args(rec)
    names = ("document", "document_ner", "document_pos", "adj_matrix", "sen_matrix", "pos_matrix_h", "pos_matrix_t", "node_pos",
             "node_type", "node_relative_pos")
    inputs = dict(zip(names, args), n_valid=rec["n_valid"], t_valid=rec["t_valid"], label_matrix=rec["label_matrix"], **kw)
    inputs["slot_records"] = rec["slot_records"].clone()

    def step_of(model):
        def step_fn(label_matrix, n_valid, **k):
            logits = model(*[k.pop(n) for n in names], n_valid=n_valid, **k)
            return gcgcn_amd.pair_bce_loss(logits, label_matrix, n_valid=n_valid).sum() / B
        return step_fn

    pg = [p for p in model_g.parameters() if p.requires_grad]
    pe = [p for p in model_e.parameters() if p.requires_grad]
    og, oe = FusedAdam(pg, lr=1e-4, capturable=True), FusedAdam(pe, lr=1e-4, capturable=True)
    train = GraphedTrainStep(step_of(model_g), og, inputs, warmup=2)
    for k, table in enumerate((rec2["slot_records"], rec["slot_records"])):
        loss_g = train(slot_records=table)
        for p in pe:
            p.grad = None
        loss_e = step_of(model_e)(**dict(inputs, slot_records=table))
        loss_e.backward()
        oe.step()
        assert torch.isfinite(loss_g).all() and torch.equal(loss_g.detach(), loss_e.detach()), f"step {k}: {loss_g.item()} != {loss_e.item()}"
    torch.cuda.synchronize()
    for (name, a), b_ in zip(model_g.state_dict().items(), model_e.state_dict().values()):
        assert torch.equal(a, b_), f"{name} differs after two steps"
