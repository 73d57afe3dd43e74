"""gcgcn_amd -- MI355X-native CAGGC + MAGGC graph-convolution blocks of GCGCN.

Drop-in ``nn.Module``s (same names / constructor args / forward signatures / state_dict keys as the
reference's ``models/GCGCN_glove.py:18-168``) whose arithmetic runs in hand-written HIP kernels for
gfx950 behind a C ABI (``include/gcgcn.h`` -> ``gcgcn_amd/lib/libgcgcn_hip.so``).  No CPU fallback.
"""
from .modules import (ClassifierHead, EdgeFeatureProducer, GraphModelTail, GATAttention, GraphConv, GraphConvolution, GraphHops,  # noqa: F401
                      MultiGraphConvolution, MultiHeadAttention)
from .functional import (TrainStats, TrainStatsResult, lstm_layer, manual_seed, pair_bce_loss, token_context,  # noqa: F401
                         token_embed)
from .bert import BertConfig, BertModel, load_pretrained_state_dict  # noqa: F401
from . import bert, evaluation, functional, models, optim, params, training  # noqa: F401
from .evaluation import EvalResult, RelationEvaluator, evaluate  # noqa: F401
from .optim import FusedAdam, GraphedTrainStep, bert_param_groups  # noqa: F401
from .training import TrainEpochResult, train_epoch  # noqa: F401

__all__ = ["BertConfig", "BertModel", "load_pretrained_state_dict", "GraphConv", "GATAttention", "MultiHeadAttention", "GraphConvolution", "MultiGraphConvolution", "GraphHops",
           "EdgeFeatureProducer", "ClassifierHead", "GraphModelTail",
           "manual_seed", "pair_bce_loss", "lstm_layer", "token_embed", "token_context", "FusedAdam", "GraphedTrainStep", "bert_param_groups", "RelationEvaluator", "EvalResult", "evaluate", "TrainStats", "TrainStatsResult", "train_epoch", "TrainEpochResult",
           "bert", "evaluation", "functional", "models", "optim", "params", "training"]
