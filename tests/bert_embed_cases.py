"""What tests/test_bert_embed_cpu.py and tests/test_bert_embed_gpu.py share: the cases of the fused embeddings stage, seeded inputs
and parameters, the runner and the float64 reference.  The bound is tests/bert_cases.py's (frac_of_bound / worst); nothing new.

The stage alone is a ``BertModel`` with NO encoder layers: ``model(ids, tt, output_all_encoded_layers=False, lengths=...)[0]`` is then
the embeddings stage's output, on every implementation.  Reference: ``impl="torch"`` in float64 on the CPU, the device's dropout mask
replayed through ``dropout_override``; computed once per case and shared (lru_cache); nobody writes to it.

A case is ``(D, B, T, extra, tt_kind, len_kind, p)``: ``Pmax = T + extra``; ``tt_kind`` "zero" | "mixed"; ``len_kind`` "none" | "full"
(all T) | "ragged" (T, 0, about T / 2, 1, ...: one document of length 0 and one of length T).  V = 11: live ids are drawn from
{0, 0, 0, 1, 1, 2, 3, 5, 6, 7, 8, 9} (rows 0 and 1 repeat many times, rows 4 and 10 never occur live); padding positions hold
id 4 or 10 -- in range, and a gradient row that must stay exactly zero if they are truly not read.  With lengths the cotangent is
NaN on padding rows.  The word table's gradient sorts chunks of 256 tokens (csrc/frontend.hip FE_CHUNK): (4, 128) = 512 tokens is
the shape that spans two chunks."""
import functools

import torch

from gcgcn_amd.bert import BertConfig, BertModel

V, TY = 11, 2
LIVE_IDS = (0, 0, 0, 1, 1, 2, 3, 5, 6, 7, 8, 9)
NEVER_LIVE = (4, 10)
HEADS = {64: 1, 128: 2, 768: 12}

CASES = [
    (64, 1, 1, 0, "zero", "none", 0.0),
    (64, 2, 5, 3, "mixed", "ragged", 0.1),
    (64, 4, 128, 0, "mixed", "none", 0.5),
    (128, 3, 33, 3, "mixed", "ragged", 0.5),
    (128, 2, 64, 0, "zero", "full", 0.1),
    (128, 3, 33, 0, "mixed", "none", 0.0),
    (768, 2, 5, 0, "mixed", "none", 0.5),
    (768, 2, 64, 3, "zero", "ragged", 0.0),
    (768, 4, 128, 3, "mixed", "ragged", 0.1),
]


def case_id(c):
    D, B, T, extra, tt, ln, p = c
    return f"D{D}-B{B}T{T}-P{T + extra}-{tt}-{ln}-p{p}"


def config(D, Pmax, p=0.0, layers=0):
    return BertConfig(vocab_size=V, hidden_size=D, num_hidden_layers=layers, num_attention_heads=HEADS[D], intermediate_size=4 * D,
                      max_position_embeddings=Pmax, type_vocab_size=TY, hidden_dropout_prob=p, attention_probs_dropout_prob=p)


@functools.lru_cache(maxsize=None)
def state(D, Pmax, layers=0):
    """A seeded float32 state_dict: tables N(0, 0.5^2), LayerNorm weight 1 + N(0, 0.1^2), bias N(0, 0.1^2) (tests/bert_cases.py)."""
    g = torch.Generator().manual_seed(300 + D + Pmax)
    sd = {}
    for k, v in BertModel(config(D, Pmax, layers=layers)).state_dict().items():
        r = torch.randn(v.shape, generator=g)
        if "LayerNorm.weight" in k:
            sd[k] = 1.0 + 0.1 * r
        elif "LayerNorm.bias" in k or k.endswith(".bias"):
            sd[k] = 0.1 * r
        elif "embeddings" in k:
            sd[k] = 0.5 * r
        else:
            sd[k] = r / v.shape[1] ** 0.5
    return sd


def lengths_of(B, T, kind):
    if kind == "none":
        return None
    if kind == "full":
        return torch.full((B,), T, dtype=torch.int64)
    assert kind == "ragged" and B >= 2
    return torch.tensor(([T, 0, T // 2 + 1, 1] * B)[:B], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def inputs(D, B, T, tt_kind, len_kind, seed=0):
    g = torch.Generator().manual_seed(7000 + 1000 * seed + 31 * B + 17 * T + D)
    ids = torch.tensor(LIVE_IDS)[torch.randint(0, len(LIVE_IDS), (B, T), generator=g)]
    tt = torch.randint(0, TY, (B, T), generator=g) if tt_kind == "mixed" else torch.zeros(B, T, dtype=torch.int64)
    dy = torch.randn(B, T, D, generator=g)
    lens = lengths_of(B, T, len_kind)
    if lens is not None:
        pad = torch.arange(T)[None, :] >= lens[:, None]
        ids = torch.where(pad, torch.tensor(NEVER_LIVE)[torch.randint(0, 2, (B, T), generator=g)], ids)
        dy = torch.where(pad[:, :, None], torch.full((), float("nan")), dy)
    return {"ids": ids, "tt": tt, "dy": dy, "lengths": lens}


GRADS = {"dW": "embeddings.word_embeddings.weight", "dP": "embeddings.position_embeddings.weight",
         "dS": "embeddings.token_type_embeddings.weight", "dweight": "embeddings.LayerNorm.weight", "dbias": "embeddings.LayerNorm.bias"}


def build(D, Pmax, p, dtype=torch.float32, device="cpu", impl="torch", embeddings="torch"):
    model = BertModel(config(D, Pmax, p), impl=impl, embeddings=embeddings)
    model.load_state_dict(state(D, Pmax), strict=True)
    return model.to(device=device, dtype=dtype)


def run_stage(model, inp, train=False, override=None, backward=True):
    """{"y", "dW", "dP", "dS", "dweight", "dbias"} of the stage alone (a model without encoder layers)."""
    dev = next(model.parameters()).device
    dtype = next(model.parameters()).dtype
    model.train(train)
    model.dropout_override = override
    model.zero_grad(set_to_none=True)
    lens = None if inp["lengths"] is None else inp["lengths"].to(dev)
    y, _ = model(inp["ids"].to(dev), inp["tt"].to(dev), output_all_encoded_layers=False, lengths=lens)
    res = {"y": y.detach()}
    if backward:
        y.backward(inp["dy"].to(device=dev, dtype=dtype))
        params = dict(model.named_parameters())
        res.update({k: params[n].grad for k, n in GRADS.items()})
    return res


def replay(snap, p):
    """dropout_override for the reference: the mask the device drew for the embeddings' site from ``snap``."""
    from gcgcn_amd import _lib, functional as Fn

    def keep(layer, site, t):
        assert (layer, site) == (-1, "emb")
        m = Fn.dropout_keep_mask(snap, _lib.SALT_BERT_EMB, p, t.numel()).view(t.shape).cpu()
        return t * m.to(t.dtype) / (1.0 - p)
    return keep


def reference(case, override=None, train=False):
    """The float64 CPU run of impl="torch" (with embeddings="fused": the same contract, the tests' reference)."""
    D, B, T, extra, tt_kind, len_kind, p = case
    model = build(D, T + extra, p, torch.float64, embeddings="fused")
    return run_stage(model, inputs(D, B, T, tt_kind, len_kind), train=train, override=override)
