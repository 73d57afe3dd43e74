"""A self-contained BERT encoder with the call contract and the ``state_dict`` keys of ``pytorch_pretrained_bert`` 0.6 ``BertModel``.

``BertModel(config, impl="torch")`` is the contract in plain PyTorch (any device, any float dtype; the reference of the tests).
``BertModel(config, impl="hip")`` runs every encoder layer through ``functional.bert_layer`` (csrc/bert.hip: masked attention
core, LayerNorm with residual and dropout, erf GELU, forward and backward, the Linears on the fp32-MFMA GEMM layer or, with
``matmul="bf16"``, on the bf16 matrix cores; the attention core's products there too with ``attention="bf16"``) and the
embeddings' LayerNorm through ``functional.res_layer_norm`` (their dropout is the library's elementwise kernel); it raises on CPU tensors.  The three embedding gathers
(word, position, token type) and the pooler (one ``[B, D] x [D, D]`` product and a tanh) stay PyTorch in both implementations:
three gathers and one small product.  ``embeddings="fused"`` moves the gathers, their sum, the LayerNorm and the dropout of
``impl="hip"`` into ``functional.bert_embeddings`` (csrc/bert_embed.hip), opt-in.  Parameters live in ordinary ``nn.Embedding`` / ``nn.Linear`` / ``nn.LayerNorm`` holders
under the package's names, so both implementations share one ``state_dict``.  DESIGN.md section 8.9."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Optional

import torch
from torch import nn
from torch.nn import functional as F

from .functional import bert_attention_index, bert_matmul_index

LN_EPS = 1e-12
MASK_PENALTY = -10000.0


@dataclass
class BertConfig:
    """bert-base-uncased by default."""
    vocab_size: int = 30522
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1


def gelu(z):
    return z * 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


def layer_norm(x, weight, bias):
    """Over the last axis, biased variance, eps = 1e-12 inside the root."""
    u = x.mean(-1, keepdim=True)
    s = (x - u).pow(2).mean(-1, keepdim=True)
    return weight * ((x - u) / torch.sqrt(s + LN_EPS)) + bias


def _holder_ln(d):
    return nn.LayerNorm(d, eps=LN_EPS)      # a parameter holder (weight, bias); the arithmetic is layer_norm() above


class _Embeddings(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.word_embeddings = nn.Embedding(c.vocab_size, c.hidden_size)
        self.position_embeddings = nn.Embedding(c.max_position_embeddings, c.hidden_size)
        self.token_type_embeddings = nn.Embedding(c.type_vocab_size, c.hidden_size)
        self.LayerNorm = _holder_ln(c.hidden_size)


class _SelfAttention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.query, self.key, self.value = (nn.Linear(c.hidden_size, c.hidden_size) for _ in range(3))


class _DenseLN(nn.Module):
    def __init__(self, n_in, n_out):
        super().__init__()
        self.dense = nn.Linear(n_in, n_out)
        self.LayerNorm = _holder_ln(n_out)


class _Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.self = _SelfAttention(c)
        self.output = _DenseLN(c.hidden_size, c.hidden_size)


class _Dense(nn.Module):
    def __init__(self, n_in, n_out):
        super().__init__()
        self.dense = nn.Linear(n_in, n_out)


class _Layer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attention = _Attention(c)
        self.intermediate = _Dense(c.hidden_size, c.intermediate_size)
        self.output = _DenseLN(c.intermediate_size, c.hidden_size)

    def tensors(self):
        """The 16 parameter tensors in functional.bert_layer's order."""
        a, o = self.attention, self.output
        return (a.self.query.weight, a.self.query.bias, a.self.key.weight, a.self.key.bias, a.self.value.weight, a.self.value.bias,
                a.output.dense.weight, a.output.dense.bias, a.output.LayerNorm.weight, a.output.LayerNorm.bias,
                self.intermediate.dense.weight, self.intermediate.dense.bias, o.dense.weight, o.dense.bias, o.LayerNorm.weight,
                o.LayerNorm.bias)


class _Encoder(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.layer = nn.ModuleList(_Layer(c) for _ in range(c.num_hidden_layers))


def _bf16(t):
    """Round every element to bfloat16 (to nearest even) and return it in the tensor's own dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


class Bf16LinearFn(torch.autograd.Function):
    """``y = bf16(x) bf16(W)^T + b`` with ``dX = bf16(dY) bf16(W)``, ``dW = bf16(dY)^T bf16(X)`` and ``db`` = the sum of the UNROUNDED
    ``dY``; the products run in the tensors' own dtype.  The definition of ``matmul="bf16"``: operands rounded once, accumulation,
    bias and everything around the product at full precision."""

    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = _bf16(x), _bf16(w)
        ctx.save_for_backward(xr, wr)
        return xr @ wr.t() + b

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dr = _bf16(dy)
        k, n = xr.shape[-1], dr.shape[-1]
        return dr @ wr, dr.reshape(-1, n).t() @ xr.reshape(-1, k), dy.reshape(-1, n).sum(0)


def bf16_linear(x, w, b):
    return Bf16LinearFn.apply(x, w, b)


class Bf16AttentionFn(torch.autograd.Function):
    """The attention core with bf16 operands, per (document, head): ``q, k, v`` ``[.., T, dh]``, ``penalty`` (additive, broadcastable
    to ``[.., T, T]``, or None), ``m`` (the multiplicative dropout mask ``keep / (1 - p)`` ``[.., T, T]``, all ones in eval mode, or
    None = ones) -> ``(ctx [.., T, dh], lse [.., T])``.  With ``r(.)`` one rounding to bfloat16 (nearest even) and ``alpha = 1 /
    sqrt(dh)``::

        S = alpha r(q) r(k)^T + penalty      P = softmax(S) over the keys, unrounded      Pd = m o P      ctx = r(Pd) r(v)
        delta_i = sum_d dctx_id ctx_id       dPd = r(dctx) r(v)^T                         dS = P o (m o dPd - delta)
        dv = r(Pd)^T r(dctx)                 dq = alpha r(dS) r(k)                        dk = alpha r(dS)^T r(q)

    The backward is stated, not derived by autograd.  Every accumulation, the softmax, ``lse``, ``delta`` and ``dS`` stay in the
    tensors' own dtype.  The definition of ``attention="bf16"``; ``lse`` takes no gradient."""

    @staticmethod
    def forward(ctx, q, k, v, penalty, m):
        alpha = 1.0 / math.sqrt(q.shape[-1])
        qr, kr, vr = _bf16(q), _bf16(k), _bf16(v)
        s = alpha * (qr @ kr.transpose(-1, -2))
        lse_shift = 0.0
        if penalty is not None:
            # a softmax does not see a shift common to its keys: the penalty enters relative to its row maximum (what the kernels do
            # with c_b), so a row whose keys are all at -10000 keeps the scores' low bits in float32; lse gets the shift back
            c = penalty.amax(-1, keepdim=True)
            s = s + (penalty - c)
            lse_shift = c.expand(s.shape[:-1] + (1,)).squeeze(-1)
        p = torch.softmax(s, dim=-1)
        lse = torch.logsumexp(s, dim=-1) + lse_shift
        pdr = _bf16(p if m is None else m * p)
        out = pdr @ vr
        ctx.alpha, ctx.has_m = alpha, m is not None
        ctx.save_for_backward(qr, kr, vr, p, pdr, out, *(() if m is None else (m,)))
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dctx, _dlse):
        qr, kr, vr, p, pdr, out = ctx.saved_tensors[:6]
        delta = (dctx * out).sum(-1, keepdim=True)
        dr = _bf16(dctx)
        dpd = dr @ vr.transpose(-1, -2)
        if ctx.has_m:
            dpd = ctx.saved_tensors[6] * dpd
        dsr = _bf16(p * (dpd - delta))
        dv = pdr.transpose(-1, -2) @ dr
        dq = ctx.alpha * (dsr @ kr)
        dk = ctx.alpha * (dsr.transpose(-1, -2) @ qr)
        return dq, dk, dv, None, None


def bf16_attention(q, k, v, penalty, m):
    """``ctx`` of ``Bf16AttentionFn``."""
    return Bf16AttentionFn.apply(q, k, v, penalty, m)[0]


def torch_layer(x, key_bias, params, heads, drop: Callable, linear: Callable = F.linear, attention: Optional[Callable] = None):
    """One encoder layer in plain PyTorch.  ``key_bias``: ``[B, T]`` additive penalty or None.  ``drop(site, t)``: the dropout of
    site "attn" (on P ``[B, H, T, T]``), "ao" or "out" (on ``[B, T, D]``).  ``linear(x, w, b)``: the six Linears (``bf16_linear`` for
    ``matmul="bf16"``).  ``attention(q, k, v, penalty, m) -> ctx [B, H, T, dh]``: None = the fp32 core written out below;
    ``bf16_attention`` for ``attention="bf16"``.  The mask is then obtained as ``m = drop("attn", ones)``, so ``drop`` must be
    MULTIPLICATIVE at that site (``drop("attn", t) == t * drop("attn", ones)``), as ``F.dropout`` and a replayed keep mask are."""
    wq, bq, wk, bk, wv, bv, wo, bo, g1, b1, wi, bi, wo2, bo2, g2, b2 = params
    B, T, D = x.shape
    dh = D // heads
    split = lambda t: t.view(B, T, heads, dh).permute(0, 2, 1, 3)
    q, k, v = split(linear(x, wq, bq)), split(linear(x, wk, bk)), split(linear(x, wv, bv))
    if attention is not None:
        m = drop("attn", torch.ones(B, heads, T, T, dtype=x.dtype, device=x.device))
        ctx = attention(q, k, v, None if key_bias is None else key_bias[:, None, None, :], m)
    else:
        s = q @ k.transpose(-1, -2) / math.sqrt(dh)
        if key_bias is not None:
            s = s + key_bias[:, None, None, :]
        p = drop("attn", torch.softmax(s, dim=-1))
        ctx = p @ v
    ctx = ctx.permute(0, 2, 1, 3).reshape(B, T, D)
    a = layer_norm(drop("ao", linear(ctx, wo, bo)) + x, g1, b1)
    i = gelu(linear(a, wi, bi))
    return layer_norm(drop("out", linear(i, wo2, bo2)) + a, g2, b2)


class BertModel(nn.Module):
    """``forward(input_ids[B,T], token_type_ids=None, attention_mask=None, output_all_encoded_layers=True) -> (encoded, pooled)``:
    ``encoded`` is the last layer's ``[B,T,D]``, or the list of every layer's output when the flag is true;
    ``pooled = tanh(pooler.dense(encoded_last[:, 0]))``.  ``attention_mask`` ``[B,T]`` (1 = a token, 0 = padding) becomes the additive
    penalty ``(1 - mask) * -10000`` on the scores: a row whose keys are all masked is a finite softmax.

    ``lengths``: the documents' token counts ``[B]`` (integers, ``0 <= lengths[b] <= T``), or None.  Row ``(b, t)`` is live iff
    ``t < lengths[b]``.  Live rows of every layer's output, and every gradient, are what the model computes for document ``b`` ALONE,
    truncated to ``lengths[b]`` tokens, with no mask; padding rows of every layer's output are exactly zero whatever token ids sit
    there, and a gradient arriving on them is ignored (NaN included).  ``attention_mask`` may still be given on top (holes inside
    the prefix).  ``pooled`` is computed from row 0 as before: for a document of length 0 that row is zero and ``pooled`` is
    ``tanh(pooler.dense.bias)``.  ``impl="hip"`` routes the lengths through the kernels (csrc/bert.hip: the attention core streams
    the live keys only, the Linears run on the live 16-row blocks, nothing is read on the host, a captured step replays on new
    lengths); ``impl="torch"`` implements the same contract as a prefix mask plus ``torch.where`` on the padding rows.  The dropout
    indices are the padded tensors', so from one snapshot the length path and the prefix-mask path drop the same live elements.

    ``dropout_override``: None, or ``f(layer, site, t) -> t`` replacing the dropout of site "emb" (layer -1), "attn", "ao", "out" of
    the torch implementation -- how a test replays the masks the HIP kernels drew.  With ``attention="bf16"`` the override of site
    "attn" is called on a tensor of ones and must be multiplicative (``f(l, "attn", t) == t * f(l, "attn", ones)``).

    ``matmul``: ``"fp32"`` (default; nothing changes) or ``"bf16"``: the six Linears of every encoder layer -- query, key, value,
    attention.output.dense, intermediate.dense, output.dense -- take bf16 operands with full-precision accumulation, forward and
    backward (``Bf16LinearFn`` is the definition: operands rounded once to nearest even, the bias gradient from the unrounded
    gradient).  Parameters, activations, gradients and ``state_dict`` stay what they are: a checkpoint moves freely between the two
    settings, and an optimizer sees fp32 master weights.  The embeddings, the attention core, LayerNorm, GELU and the pooler are
    unchanged.  ``impl="hip"`` hands the selector to every layer (csrc/gemm_bf16.hip: the bf16 matrix cores); ``impl="torch"`` is the
    same contract on any device and float dtype.

    ``attention``: ``"fp32"`` (default; nothing changes) or ``"bf16"``: the attention core's four matrix products -- ``q k^T``,
    ``P v`` and in the backward ``dctx v^T``, ``dS k`` / ``dS^T q`` / ``P^T dctx`` -- take bf16 operands with full-precision
    accumulation; softmax, ``lse``, ``delta`` and ``dS`` stay at full precision and the dropout mask is the one the fp32 core draws
    (``Bf16AttentionFn`` is the definition).  Independent of ``matmul``: all four combinations are valid, and a checkpoint moves
    freely between them.  ``impl="hip"``: csrc/bert_attn_bf16.hip.  After a training forward of ``impl="hip"``,
    ``last_rng_snaps`` holds the snapshots it used: ``[0]`` for the embeddings, ``[1 + l]`` for layer ``l``.

    ``embeddings``: ``"torch"`` (default; nothing changes, launch for launch) or ``"fused"``: with ``impl="hip"`` the stage in front
    of the layers -- ``(word[ids] + position[t]) + type[token_type_ids]``, LayerNorm, dropout, zeros on padding rows -- is ONE launch
    of ``functional.bert_embeddings`` (csrc/bert_embed.hip) that never stores the sum, and its backward computes the three tables'
    gradients owner-computed, dense and bit-reproducible; ids at padding positions are not read.  The forward is bit for bit the
    default's (the same two fp32 adds, the same LayerNorm row body, the same dropout mask).  ``impl="torch"`` accepts the value and
    computes the same contract in plain PyTorch as it always did.  Independent of ``matmul`` and ``attention``; the ``state_dict`` is
    untouched, so a checkpoint moves freely between the settings."""

    def __init__(self, config: Optional[BertConfig] = None, impl: str = "torch", matmul: str = "fp32", attention: str = "fp32",
                 embeddings: str = "torch"):
        super().__init__()
        config = BertConfig() if config is None else config
        if impl not in ("torch", "hip"):
            raise ValueError(f"BertModel: impl must be 'torch' or 'hip', got {impl!r}")
        bert_matmul_index(matmul, "BertModel")      # raises on anything but the allowed names
        bert_attention_index(attention, "BertModel")
        if embeddings not in ("torch", "fused"):
            raise ValueError(f"BertModel: embeddings must be 'torch' or 'fused', got {embeddings!r}")
        if config.hidden_size % config.num_attention_heads:
            raise ValueError(f"BertModel: hidden size {config.hidden_size} is no multiple of {config.num_attention_heads} heads")
        if impl == "hip" and config.hidden_size != 64 * config.num_attention_heads:
            raise ValueError(f"BertModel(impl='hip'): the attention kernels serve a head width of 64, not "
                             f"{config.hidden_size // config.num_attention_heads}")
        self.config, self.impl, self.matmul, self.attention = config, impl, matmul, attention
        self.embeddings_impl = embeddings           # (self.embeddings is the parameters' holder: a state_dict key)
        self.embeddings = _Embeddings(config)
        self.encoder = _Encoder(config)
        self.pooler = _Dense(config.hidden_size, config.hidden_size)
        self.dropout_override = None
        self.last_rng_snaps = None
        self.apply(self._init)

    @staticmethod
    def _init(m):   # pytorch_pretrained_bert's init_bert_weights
        if isinstance(m, (nn.Linear, nn.Embedding)):
            m.weight.data.normal_(mean=0.0, std=0.02)
        if isinstance(m, nn.Linear) and m.bias is not None:
            m.bias.data.zero_()

    def _drop(self, layer, site, t, p):
        if self.dropout_override is not None:
            return self.dropout_override(layer, site, t)
        return F.dropout(t, p, self.training)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, output_all_encoded_layers=True, lengths=None):
        c, e = self.config, self.embeddings
        B, T = input_ids.shape
        if lengths is not None and tuple(lengths.shape) != (B,):
            raise ValueError(f"BertModel: lengths {tuple(lengths.shape)}, expected ({B},)")
        if T > c.max_position_embeddings:
            raise ValueError(f"BertModel: {T} tokens exceed max_position_embeddings = {c.max_position_embeddings}")
        tt = torch.zeros_like(input_ids) if token_type_ids is None else token_type_ids
        if self.impl == "hip" and self.embeddings_impl == "fused":      # the sum is formed inside the stage's kernel
            dt = e.word_embeddings.weight.dtype
            key_bias = None if attention_mask is None else (1.0 - attention_mask.to(dt)) * MASK_PENALTY
            outs = self._encode_hip(None, key_bias, lengths, ids=input_ids, tt=tt)
            pooled = torch.tanh(self.pooler.dense(outs[-1][:, 0]))
            return (outs if output_all_encoded_layers else outs[-1]), pooled
        pos = torch.arange(T, device=input_ids.device)
        emb = e.word_embeddings(input_ids) + e.position_embeddings(pos)[None] + e.token_type_embeddings(tt)
        key_bias = None if attention_mask is None else (1.0 - attention_mask.to(emb.dtype)) * MASK_PENALTY
        if self.impl == "hip":
            outs = self._encode_hip(emb, key_bias, lengths)
        else:
            live = None
            if lengths is not None:     # the contract in plain PyTorch: a prefix mask on the keys, padding rows selected away
                live = torch.arange(T, device=emb.device)[None, :] < lengths.to(emb.device)[:, None]
                prefix = (~live).to(emb.dtype) * MASK_PENALTY      # exp(-10000 - max) is exactly 0 in float32 and in float64
                key_bias = prefix if key_bias is None else key_bias + prefix
                live = live[:, :, None]
            # torch.where, not a product: its backward hands the unselected branch a zero whatever arrives, NaN included
            zero_pad = (lambda t: t) if live is None else (lambda t: torch.where(live, t, torch.zeros((), dtype=t.dtype, device=t.device)))
            x = zero_pad(self._drop(-1, "emb", layer_norm(emb, e.LayerNorm.weight, e.LayerNorm.bias), c.hidden_dropout_prob))
            outs = []
            linear = {"linear": bf16_linear} if self.matmul == "bf16" else {}      # "fp32": the call as it was
            if self.attention == "bf16":
                linear["attention"] = bf16_attention
            for li, layer in enumerate(self.encoder.layer):
                probs = {"attn": c.attention_probs_dropout_prob, "ao": c.hidden_dropout_prob, "out": c.hidden_dropout_prob}
                x = zero_pad(torch_layer(x, key_bias, layer.tensors(), c.num_attention_heads, lambda s, t: self._drop(li, s, t, probs[s]),
                                         **linear))
                outs.append(x)
        last = outs[-1] if outs else x
        pooled = torch.tanh(self.pooler.dense(last[:, 0]))
        return (outs if output_all_encoded_layers else last), pooled

    def _encode_hip(self, emb, key_bias, lengths=None, ids=None, tt=None):
        """``emb``: the embeddings' sum ``[B,T,D]``; or None with ``ids`` / ``tt`` ``[B,T]`` (``embeddings="fused"``)."""
        from . import _lib, functional as Fn
        c, e = self.config, self.embeddings
        src = ids if emb is None else emb
        if not src.is_cuda:
            raise RuntimeError(f"BertModel(impl='hip') runs on MI355X only; got {src.device} tensors (impl='torch' runs anywhere)")
        dev, (B, T) = src.device, src.shape[:2]
        training = self.training
        n = len(self.encoder.layer)
        snaps = []
        tv = rowblk = None
        if lengths is not None:      # one list of live 16-row blocks for every layer and its backward, built on the device
            tv = lengths.to(device=dev, dtype=torch.int32).contiguous()
            rowblk = Fn.row_blocks(tv, B, T)
        with Fn.rng_scope(dev, n + 1, enabled=training):
            snap = Fn.rng_snapshot(dev) if training and c.hidden_dropout_prob > 0 else None
            snaps.append(snap)
            if emb is None:
                x = Fn.bert_embeddings(ids, tt, e.word_embeddings.weight, e.position_embeddings.weight, e.token_type_embeddings.weight,
                                       e.LayerNorm.weight, e.LayerNorm.bias, p=c.hidden_dropout_prob, training=snap is not None, snap=snap,
                                       t_valid=tv)
            else:
                # the dropout follows the LayerNorm here; with lengths the LayerNorm zeroes the padding rows and the dropout keeps 0 at 0
                x = Fn.res_layer_norm(emb, e.LayerNorm.weight, e.LayerNorm.bias, t_valid=tv)
                if snap is not None:
                    x = Fn.DropoutFn.apply(x, c.hidden_dropout_prob, snap, _lib.SALT_BERT_EMB)
            outs = []
            kb = None if key_bias is None else key_bias.contiguous()
            for layer in self.encoder.layer:
                snap = Fn.rng_snapshot(dev) if training else None
                snaps.append(snap)
                x = Fn.bert_layer(x, kb, *layer.tensors(), p_attn=c.attention_probs_dropout_prob, p_hidden=c.hidden_dropout_prob,
                                  training=training, snap=snap, t_valid=tv, rowblk=rowblk, matmul=self.matmul, attention=self.attention)
                outs.append(x)
        self.last_rng_snaps = snaps if training else None
        if not outs:
            outs = [x]
        return outs


def load_pretrained_state_dict(model: nn.Module, path: str, strict: bool = True):
    """Load a LOCAL checkpoint file (``torch.load``; nothing is downloaded) into ``model``.  Checkpoints of the original TensorFlow
    conversion spell the LayerNorm parameters ``gamma`` / ``beta``: they are renamed to ``weight`` / ``bias``.  A ``bert.`` prefix
    (a checkpoint of a model that wraps the encoder) is dropped when every key carries it."""
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd and not any(torch.is_tensor(v) for v in sd.values()):
        sd = sd["state_dict"]
    if sd and all(k.startswith("bert.") for k in sd):
        sd = {k[len("bert."):]: v for k, v in sd.items()}
    return model.load_state_dict(rename_gamma_beta(sd), strict=strict)


def rename_gamma_beta(sd: dict) -> dict:
    out = {}
    for k, v in sd.items():
        if k.endswith(".gamma"):
            k = k[:-len("gamma")] + "weight"
        elif k.endswith(".beta"):
            k = k[:-len("beta")] + "bias"
        out[k] = v
    return out
