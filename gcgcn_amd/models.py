"""Model-level drop-ins: the classes ``config/Config.py`` instantiates (``model_pattern(config=self)``, Config.py:294) and
calls with the ten tensors of ``Config.from_list_to_tensor`` (Config.py:354), same constructor, ``forward`` signature and
``state_dict`` keys as the reference's

    GCGCN_glove                           /root/reference/models/GCGCN_glove.py:215-360
    GraphCNN_multihead_bert_gate_cls      /root/reference/models/GraphCNN_multihead_bert_gate_cls.py:219-351

so that ``con.train(gcgcn_amd.models.GCGCN_glove, save_name)`` runs the reference's trainer unchanged and a reference
checkpoint loads with ``strict=True``.

What runs where.  Everything from the entity pooling on (glove:293-360: edge-feature producers, CAGGC / MAGGC blocks, hop glue,
classifier head) is :class:`gcgcn_amd.GraphModelTail`, i.e. the HIP kernels.  The token encoder in front of it -- embeddings,
``EncoderLSTM`` (glove:377-428), ``linear_re`` + tanh, or BERT in the second model -- is plain PyTorch by default, restated here
so that the model is complete.  ``config.encoder_impl = "hip"`` opts the BiLSTM into ``functional.lstm_layer``;
``config.encoder_recurrent = "bf16"`` (needs ``encoder_impl``; a ``ValueError`` without it) gives its recurrent products bf16 operands;
``config.frontend_impl = "hip"``, independently, opts the embeddings with their locked dropout into ``functional.token_embed`` and
``linear_re`` + tanh + the entity pooling into ``functional.token_context``.

Extension: every ``forward`` also accepts a leading batch axis on all ten tensors (what ``gcgcn_amd.data.collate`` returns)
plus ``n_valid[B]``; the reference's one-document call (``document[T]``, ``sen_matrix[N,N,S,T]`` ...) behaves as the reference's.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from .bert import BertModel as OwnBertModel
from .functional import bert_token_context, lstm_layer, lstm_layer_bf16_definition, pair_logit_bias, token_context, token_embed
from .modules import GraphModelTail

Tensor = torch.Tensor


class LockedDropout(nn.Module):
    """One mask per (batch entry, feature), shared by all time steps (glove:363-375); identity in eval mode."""

    def __init__(self, dropout: float):
        super().__init__()
        self.dropout = float(dropout)

    def factor(self, batch: int, features: int, dtype, device) -> Optional[Tensor]:
        """The mask over ``[batch, 1, features]`` divided by the keep probability, or ``None`` where ``forward`` is the identity."""
        if not self.training or self.dropout <= 0.0:
            return None
        keep = 1.0 - self.dropout
        return torch.empty(batch, 1, features, dtype=dtype, device=device).bernoulli_(keep) / keep

    def forward(self, x: Tensor) -> Tensor:
        m = self.factor(x.size(0), x.size(2), x.dtype, x.device)
        return x if m is None else m.expand_as(x) * x


class EncoderLSTM(nn.Module):
    """The reference's BiLSTM token encoder (glove:377-428): ``nlayers`` ``nn.LSTM``s with learned initial states, locked dropout
    in front of every layer, layer outputs concatenated.  Parameter names as in the reference: ``rnns.{i}.*``, ``init_hidden.{i}``,
    ``init_c.{i}``.  ``impl="torch"`` (the default) is plain PyTorch (MIOpen's LSTM on ROCm); ``impl="hip"`` runs every layer
    through ``functional.lstm_layer`` on the same parameters -- the ``nn.LSTM`` modules stay as their holders, so the
    ``state_dict`` is the same either way -- and raises on CPU tensors.

    ``forward(input, input_lengths)``: a TENSOR ``input_lengths`` (int ``[B]``, values in ``[1, T]``) makes every layer run each
    row at its own length, as a packed sequence: ``impl="hip"`` hands it to ``lstm_layer``, ``impl="torch"`` packs and pads back to
    ``T`` (the output is 0 past a row's length).  Anything else there (the reference passes ``doc.size(1)``) is ignored.

    ``recurrent="bf16"`` (default ``"fp32"``) gives the layers' two recurrent products bf16 operands with fp32 accumulation;
    parameters, gradients and the ``state_dict`` stay fp32, so a checkpoint moves freely between the settings.  ``impl="hip"``
    hands it to ``lstm_layer``; ``impl="torch"`` then runs ``functional.lstm_layer_bf16_definition``, the same contract as a Python
    time loop (any device, tensor lengths honoured; slow)."""

    def __init__(self, input_size, num_units, nlayers, concat, bidir, dropout, return_last, impl="torch", recurrent="fp32"):
        super().__init__()
        if impl not in ("torch", "hip"):
            raise ValueError(f"EncoderLSTM: impl={impl!r} (\"torch\" or \"hip\")")
        if recurrent not in ("fp32", "bf16"):
            raise ValueError(f"EncoderLSTM: recurrent={recurrent!r} (\"fp32\" or \"bf16\")")
        self.impl, self.recurrent = impl, recurrent
        self.rnns = nn.ModuleList(nn.LSTM(input_size if i == 0 else (num_units * 2 if bidir else num_units), num_units, 1,
                                          bidirectional=bidir, batch_first=True) for i in range(nlayers))
        nd = 2 if bidir else 1
        self.init_hidden = nn.ParameterList([nn.Parameter(torch.zeros(nd, 1, num_units)) for _ in range(nlayers)])
        self.init_c = nn.ParameterList([nn.Parameter(torch.zeros(nd, 1, num_units)) for _ in range(nlayers)])
        self.dropout = LockedDropout(dropout)
        self.concat, self.nlayers, self.return_last = concat, nlayers, return_last

    def forward(self, input: Tensor, input_lengths=None, input_dropped: bool = False) -> Tensor:
        """``input_dropped``: the caller has applied the first layer's locked dropout to ``input`` already (``token_embed``'s scale)."""
        bsz = input.size(0)
        lengths = input_lengths if isinstance(input_lengths, Tensor) else None
        output, outputs = input, []
        for i in range(self.nlayers):
            drop = (lambda x: x) if i == 0 and input_dropped else self.dropout
            if self.impl == "hip" or self.recurrent == "bf16":
                r = self.rnns[i]
                rev = (r.weight_ih_l0_reverse, r.weight_hh_l0_reverse, r.bias_ih_l0_reverse, r.bias_hh_l0_reverse) if r.bidirectional else ()
                if self.impl == "hip":
                    output = lstm_layer(drop(output), r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0,
                                        self.init_hidden[i], self.init_c[i], *rev, lengths=lengths,
                                        **({} if self.recurrent == "fp32" else {"recurrent": self.recurrent}))
                else:
                    output = lstm_layer_bf16_definition(drop(output), r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0,
                                                        self.init_hidden[i], self.init_c[i], *rev, lengths=lengths)
                outputs.append(output)
                continue
            h0 = self.init_hidden[i].expand(-1, bsz, -1).contiguous()
            c0 = self.init_c[i].expand(-1, bsz, -1).contiguous()
            if lengths is not None:                   # torch wants the lengths on the host
                packed = pack_padded_sequence(drop(output), lengths.cpu(), batch_first=True, enforce_sorted=False)
                output, _ = pad_packed_sequence(self.rnns[i](packed, (h0, c0))[0], batch_first=True, total_length=input.size(1))
                outputs.append(output)
                continue
            output, _ = self.rnns[i](drop(output), (h0, c0))
            outputs.append(output)
        return torch.cat(outputs, dim=2) if self.concat else outputs[-1]


class _GraphRelationModel(GraphModelTail):
    """What the two models share: construction of the post-encoder part, the reference's key order in ``state_dict()``, and
    ``forward`` from the encoder's token states on."""

    HIDDEN = 128                       # hard-coded in both reference models (glove:234, bert:237)
    _KEY_ORDER = ()                    # top-level attribute names in the reference's registration order

    def __init__(self, config, layer_num: int, head_num: int):
        super().__init__(hidden_size=self.HIDDEN, layer_num=layer_num, head_num=head_num, graph_hop=config.graph_hop,
                         alpha=config.alpha, dis_size=config.dis_size, entity_type_size=config.entity_type_size,
                         relation_num=config.relation_num, dis_plus=config.dis_plus, dropout=0.2,
                         head_matmul=getattr(config, "head_matmul", "fp32"))   # "fp32" | "bf16": ClassifierHead's matmul
        self.config = config
        self.frontend_impl = getattr(config, "frontend_impl", "torch")
        if self.frontend_impl not in ("torch", "hip"):
            raise ValueError(f"config.frontend_impl={self.frontend_impl!r} (\"torch\" or \"hip\")")
        self.deterministic = bool(getattr(config, "deterministic", False))   # GraphModelTail.deterministic: bit-reproducible producers
        self.layerNum, self.headNum = layer_num, head_num
        self._register_state_dict_hook(self._reference_order_hook)

    # keys come out grouped the way the reference registers its attributes (the key SET is what load_state_dict needs; the
    # order only matters to code that zips two state dicts)
    @staticmethod
    def _reference_order_hook(module, state_dict, prefix, local_metadata):
        rank = {name: i for i, name in enumerate(module._KEY_ORDER)}
        items = list(state_dict.items())
        mine = [(k, v) for k, v in items if k.startswith(prefix)]
        keyed = sorted(range(len(mine)), key=lambda i: (rank.get(mine[i][0][len(prefix):].split(".", 1)[0], len(rank)), i))
        state_dict.clear()
        for k, v in items:
            if not k.startswith(prefix):
                state_dict[k] = v
        for i in keyed:
            state_dict[mine[i][0]] = mine[i][1]

    def _graph_forward(self, context_output, adj_matrix, sen_matrix, pos_matrix_h, pos_matrix_t, node_pos, node_type,
                       node_relative_pos, n_valid, batched, node_feat=None, **caps):
        # entity pooling (glove:293-298): node_feat[n] = sum_t node_pos[n, t] * context_output[t]; the hip front end hands it in
        if node_feat is None:
            node_feat = torch.bmm(node_pos, context_output) if batched else node_pos @ context_output.squeeze(0)
        return GraphModelTail.forward(self, context_output, node_feat, adj_matrix, sen_matrix, pos_matrix_h, pos_matrix_t, node_type,
                                      node_relative_pos, self.dis_embed.weight, self.ner_emb.weight, n_valid=n_valid, **caps)


class GCGCN_glove(_GraphRelationModel):
    """``GCGCN_glove(config)`` (glove:215-360).  ``config`` carries what the reference's does: ``data_word_vec`` (numpy
    ``[V, 100]``), ``entity_type_size``, ``coref_size``, ``max_length``, ``keep_prob``, ``graph_hop``, ``dis_size``, ``dis_num``,
    ``dis_plus``, ``relation_num``, ``alpha``."""

    _KEY_ORDER = ("word_emb", "ner_emb", "entity_embed", "rnn", "get_weighted_adj_matrix", "get_adj_matrix", "graphcnn", "linear_re",
                  "word_attention", "sentence_attention", "linear_word_att", "linear_sentence_att", "dense_layer", "bili_layer_01",
                  "classification_layer_01", "dis_embed")

    def __init__(self, config):
        super().__init__(config, layer_num=2, head_num=8)                                   # glove:250-251
        vec = np.asarray(config.data_word_vec, dtype=np.float32)
        self.word_emb = nn.Embedding(vec.shape[0], vec.shape[1])                             # glove:220-223
        self.word_emb.weight.data.copy_(torch.from_numpy(vec))
        self.word_emb.weight.requires_grad = True
        input_size = vec.shape[1] + config.entity_type_size + config.coref_size
        self.ner_emb = nn.Embedding(7, config.entity_type_size, padding_idx=0)               # glove:241
        self.entity_embed = nn.Embedding(config.max_length, config.coref_size, padding_idx=0)   # glove:246
        recurrent = getattr(config, "encoder_recurrent", "fp32")
        if recurrent == "bf16" and getattr(config, "encoder_impl", None) is None:
            raise ValueError("config.encoder_recurrent selects the recurrent products of EncoderLSTM's impl: set config.encoder_impl too")
        self.rnn = EncoderLSTM(input_size, self.HIDDEN, 1, True, True, 1 - config.keep_prob, False,   # glove:248
                               impl=getattr(config, "encoder_impl", "torch"), recurrent=recurrent)
        self.linear_re = nn.Linear(self.HIDDEN * 2, self.HIDDEN)                             # glove:264
        self.dis_embed = nn.Embedding(config.dis_num, config.dis_size)                       # glove:279

    def encode(self, document: Tensor, document_ner: Tensor, document_pos: Tensor, t_valid: Optional[Tensor] = None) -> Tensor:
        """Token states ``context_output`` ``[B,T,128]`` (glove:282-292).  ``t_valid``: the documents' token counts ``[B]``
        (``data.collate``); the encoder then runs each document at its own length."""
        if self.frontend_impl == "hip":
            return self._encode_pooled(document, document_ner, document_pos, document.new_zeros(document.size(0), 1, document.size(1),
                                                                                                dtype=torch.float32), t_valid)[0]
        doc = torch.cat([self.word_emb(document), self.entity_embed(document_pos), self.ner_emb(document_ner)], dim=-1)
        return torch.tanh(self.linear_re(self.rnn(doc, doc.size(1) if t_valid is None else t_valid)))

    def _encode_pooled(self, document, document_ner, document_pos, node_pos, t_valid=None):
        """The hip front end: ``(context_output [B,T,128], node_feat [B,N,128])``.  The locked dropout in front of the first LSTM
        layer is drawn here, by the same torch call, and applied inside ``token_embed``."""
        I = self.word_emb.embedding_dim + self.entity_embed.embedding_dim + self.ner_emb.embedding_dim
        scale = self.rnn.dropout.factor(document.size(0), I, self.word_emb.weight.dtype, document.device)
        doc = token_embed(document, document_pos, document_ner, self.word_emb.weight, self.entity_embed.weight, self.ner_emb.weight,
                          scale, self.entity_embed.padding_idx, self.ner_emb.padding_idx)
        h = self.rnn(doc, doc.size(1) if t_valid is None else t_valid, input_dropped=True)
        return token_context(h, self.linear_re.weight, self.linear_re.bias, node_pos)

    def forward(self, document, document_ner, document_pos, adj_matrix, sen_matrix, pos_matrix_h, pos_matrix_t, node_pos, node_type,
                node_relative_pos, n_valid: Optional[Tensor] = None, t_valid: Optional[Tensor] = None, **caps):
        """``t_valid``: the token count of every document of a batch, ``[B]`` (``data.collate`` returns it).  With it the BiLSTM
        runs each document at its own length, which is what the one-document call computes; without it every document runs all
        ``T`` padded steps."""
        batched = document.dim() == 2
        if not batched:
            document, document_ner, document_pos = (t.unsqueeze(0) for t in (document, document_ner, document_pos))
        node_feat = None
        if self.frontend_impl == "hip":
            ctx, node_feat = self._encode_pooled(document, document_ner, document_pos, node_pos if batched else node_pos.unsqueeze(0),
                                                 t_valid)
            node_feat = node_feat if batched else node_feat[0]
        else:
            ctx = self.encode(document, document_ner, document_pos, t_valid)
        return self._graph_forward(ctx, adj_matrix, sen_matrix, pos_matrix_h, pos_matrix_t, node_pos, node_type, node_relative_pos,
                                   n_valid, batched, node_feat=node_feat, **caps)


class GraphCNN_multihead_bert_gate_cls(_GraphRelationModel):
    """The BERT variant (bert:219-351): token states from ``BertModel`` instead of the BiLSTM, four sub-layers and four heads,
    and ``linear_cls`` of the [CLS] state added to every pair's logits (bert:345-346).

    ``bert``: the encoder module, called as the reference calls it -- ``bert(document[B,T], output_all_encoded_layers=False)`` ->
    ``(states[B,T,768], pooled)``.  Default: ``pytorch_pretrained_bert.BertModel.from_pretrained('./bert/bert-base-uncased')``
    exactly as bert:228; that package / those weights are third-party and are not part of this library, so without them the
    constructor raises ImportError unless an encoder is passed in.

    ``config.bert_impl = "torch" | "hip"`` builds this library's own encoder instead: ``gcgcn_amd.BertModel(config.bert_config or
    BertConfig(), impl=...)``, its weights loaded from the LOCAL file ``config.bert_weights`` when that is set; the token width
    follows ``bert_config.hidden_size``.  Without ``bert_impl`` nothing changes.

    ``config.bert_matmul = "fp32" | "bf16"`` (needs ``bert_impl``; a ``ValueError`` without it) is that encoder's ``matmul``: with
    ``"bf16"`` the encoder layers' Linears take bf16 operands with fp32 accumulation while parameters, gradients and the
    ``state_dict`` stay fp32 (``gcgcn_amd.BertModel``).  Without ``bert_matmul`` nothing changes.

    ``config.bert_attention = "fp32" | "bf16"`` (needs ``bert_impl``; a ``ValueError`` without it) is that encoder's ``attention``:
    with ``"bf16"`` the attention core's four matrix products take bf16 operands as well (``gcgcn_amd.bert.Bf16AttentionFn`` is the
    definition).  Independent of ``bert_matmul``.  Without ``bert_attention`` nothing changes.

    ``config.bert_embeddings = "torch" | "fused"`` (needs ``bert_impl``; a ``ValueError`` without it) is that encoder's
    ``embeddings``: with ``"fused"`` and ``bert_impl = "hip"`` the stage in front of the layers -- three gathers, their sum,
    LayerNorm, dropout -- is one launch, with owner-computed, bit-reproducible table gradients (``functional.bert_embeddings``).
    Independent of ``bert_matmul`` and ``bert_attention``.  Without ``bert_embeddings`` nothing changes.

    ``config.bert_frontend = "cat" | "folded"`` (``"folded"`` needs ``config.frontend_impl = "hip"``; a ``ValueError`` without it) is
    this model's own glue either side of the tail.  ``"folded"`` runs ``functional.bert_token_context`` -- the two small tables folded
    through ``linear_re``, no ``[B,T,808]`` tensor in either direction, owner-computed bit-reproducible table gradients -- and adds
    ``linear_cls`` of the [CLS] state with ``functional.pair_logit_bias`` (one launch; ``dcls`` in a fixed order).  Parameters and the
    ``state_dict`` are the same either way.  ``"cat"``, or no ``bert_frontend``, changes nothing."""

    WORD_VEC_SIZE = 768
    _KEY_ORDER = ("bert", "ner_emb", "entity_embed", "get_weighted_adj_matrix", "get_adj_matrix", "graphcnn", "linear_re",
                  "word_attention", "sentence_attention", "linear_word_att", "linear_sentence_att", "dense_layer", "bili_layer_01",
                  "classification_layer_01", "linear_cls", "dis_embed")

    def __init__(self, config, bert: Optional[nn.Module] = None):
        super().__init__(config, layer_num=4, head_num=4)                                   # bert:247-248
        impl = getattr(config, "bert_impl", None)
        matmul = getattr(config, "bert_matmul", None)
        if matmul is not None:
            if matmul not in ("fp32", "bf16"):
                raise ValueError(f"config.bert_matmul must be 'fp32' or 'bf16', got {matmul!r}")
            if impl is None:
                raise ValueError("config.bert_matmul selects the Linears of this library's own encoder: set config.bert_impl too")
        attention = getattr(config, "bert_attention", None)
        if attention is not None:
            if attention not in ("fp32", "bf16"):
                raise ValueError(f"config.bert_attention must be 'fp32' or 'bf16', got {attention!r}")
            if impl is None:
                raise ValueError("config.bert_attention selects the attention core of this library's own encoder: set config.bert_impl too")
        embeddings = getattr(config, "bert_embeddings", None)
        if embeddings is not None:
            if embeddings not in ("torch", "fused"):
                raise ValueError(f"config.bert_embeddings must be 'torch' or 'fused', got {embeddings!r}")
            if impl is None:
                raise ValueError("config.bert_embeddings selects the embeddings stage of this library's own encoder: set config.bert_impl too")
        self.bert_frontend = getattr(config, "bert_frontend", "cat")
        if self.bert_frontend not in ("cat", "folded"):
            raise ValueError(f"config.bert_frontend must be 'cat' or 'folded', got {self.bert_frontend!r}")
        if self.bert_frontend == "folded" and self.frontend_impl != "hip":
            raise ValueError("config.bert_frontend='folded' selects kernels of the hip front end: set config.frontend_impl='hip' too")
        if bert is None and impl is not None:                                                # this library's own encoder (bert.py)
            from .bert import BertConfig, BertModel as OwnBert, load_pretrained_state_dict
            if impl not in ("torch", "hip"):
                raise ValueError(f"config.bert_impl must be 'torch' or 'hip', got {impl!r}")
            bert = OwnBert(getattr(config, "bert_config", None) or BertConfig(), impl=impl, **({} if matmul is None else {"matmul": matmul}),
                           **({} if attention is None else {"attention": attention}),
                           **({} if embeddings is None else {"embeddings": embeddings}))
            if getattr(config, "bert_weights", None):
                load_pretrained_state_dict(bert, config.bert_weights)
            if bert.config.hidden_size != self.WORD_VEC_SIZE:
                self.WORD_VEC_SIZE = bert.config.hidden_size
        if bert is None:
            try:
                from pytorch_pretrained_bert import BertModel
            except ImportError as e:
                raise ImportError("GraphCNN_multihead_bert_gate_cls needs an encoder: install pytorch_pretrained_bert with "
                                  "./bert/bert-base-uncased (bert:228), or pass bert=<module>") from e
            bert = BertModel.from_pretrained("./bert/bert-base-uncased")
        self.bert = bert
        input_size = self.WORD_VEC_SIZE + config.entity_type_size + config.coref_size
        self.ner_emb = nn.Embedding(7, config.entity_type_size, padding_idx=0)
        self.entity_embed = nn.Embedding(config.max_length, config.coref_size, padding_idx=0)
        self.linear_re = nn.Linear(input_size, self.HIDDEN)                                  # bert:259
        self.linear_cls = nn.Linear(self.WORD_VEC_SIZE, config.relation_num)                 # bert:270
        self.dis_embed = nn.Embedding(config.dis_num, config.dis_size)

    def forward(self, document, document_ner, document_pos, adj_matrix, sen_matrix, pos_matrix_h, pos_matrix_t, node_pos, node_type,
                node_relative_pos, n_valid: Optional[Tensor] = None, t_valid: Optional[Tensor] = None, **caps):
        """``t_valid``: the token count of every document of a batch, ``[B]``.  This library's own encoder (``config.bert_impl``) is
        called with ``lengths=t_valid``: each document runs at its own token count and the token states of padding rows are exactly
        zero -- ``impl="hip"`` in the kernels, on live tokens only; ``impl="torch"`` by the same contract in plain PyTorch, so the two
        stay interchangeable on every row.  Any other encoder is called with ``attention_mask = arange(T) < t_valid[:, None]`` as
        before, so that real tokens do not attend to padding."""
        batched = document.dim() == 2
        if not batched:
            document, document_ner, document_pos = (t.unsqueeze(0) for t in (document, document_ner, document_pos))
        if t_valid is None:
            doc, _ = self.bert(document, output_all_encoded_layers=False)                    # bert:275
        elif isinstance(self.bert, OwnBertModel):
            doc, _ = self.bert(document, output_all_encoded_layers=False, lengths=t_valid)
        else:
            mask = torch.arange(document.size(1), device=document.device) < t_valid.to(document.device)[:, None]
            doc, _ = self.bert(document, attention_mask=mask, output_all_encoded_layers=False)
        cls_feat = doc[:, 0, :]                                                              # bert:277
        if self.bert_frontend == "folded":
            ctx, node_feat = bert_token_context(doc, document_pos, document_ner, self.entity_embed.weight, self.ner_emb.weight,
                                                self.linear_re.weight, self.linear_re.bias, node_pos if batched else node_pos.unsqueeze(0),
                                                self.entity_embed.padding_idx, self.ner_emb.padding_idx)
            logits = self._graph_forward(ctx, adj_matrix, sen_matrix, pos_matrix_h, pos_matrix_t, node_pos, node_type, node_relative_pos,
                                         n_valid, batched, node_feat=node_feat if batched else node_feat[0], **caps)
            cls = self.linear_cls(cls_feat)                                                  # bert:345
            return pair_logit_bias(logits, cls, n_valid) if batched else pair_logit_bias(logits.unsqueeze(0), cls)[0]
        doc = torch.cat([doc, self.entity_embed(document_pos), self.ner_emb(document_ner)], dim=-1)
        node_feat = None
        if self.frontend_impl == "hip":
            ctx, node_feat = token_context(doc, self.linear_re.weight, self.linear_re.bias, node_pos if batched else node_pos.unsqueeze(0))
            node_feat = node_feat if batched else node_feat[0]
        else:
            ctx = torch.tanh(self.linear_re(doc))                                            # bert:283
        logits = self._graph_forward(ctx, adj_matrix, sen_matrix, pos_matrix_h, pos_matrix_t, node_pos, node_type,
                                     node_relative_pos, n_valid, batched, node_feat=node_feat, **caps)
        cls = self.linear_cls(cls_feat)                                                      # bert:345
        if not batched:
            return logits + cls[0]
        add = cls[:, None, None, :]
        if n_valid is not None:                  # padding pairs of a ragged batch stay zero
            ok = torch.arange(logits.shape[1], device=logits.device)[None, :] < n_valid[:, None]
            add = add * (ok[:, :, None] & ok[:, None, :]).unsqueeze(-1).to(add.dtype)
        return logits + add
