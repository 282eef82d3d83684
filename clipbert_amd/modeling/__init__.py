"""ClipBERT module API on top of libclipbert_hip (MI355X / gfx950).

The classes keep the reference's names, constructor / forward signatures, returned dicts and
state-dict keys:

    ClipBert(config, input_format="BGR", detectron2_model_cfg=..., transformer_cls=...)   e2e_model.py:14-50
    GridFeatBackbone                                                                      grid_feat.py:37-105
    ClipBertForPreTraining / ...VideoTextRetrieval / ...MultipleChoice / ...SequenceClassification
                                                                                          modeling.py:241-580

but they hold no PyTorch compute: parameters are views into flat HBM buffers (params.ParamBank) and
every forward / backward step is a call into the C ABI (clipbert_amd.ops).  The backward pass is written
out explicitly (two coarse autograd nodes: CNN trunk, cross-modal encoder) so that residual-gradient
sums, ReLU/FrozenBN masks and bias/LayerNorm reductions are fused into kernel epilogues instead of
being left to autograd's eager tensor ops.  Parameter gradients are accumulated by the kernels
directly into the flat fp32 gradient buffer (``p.grad`` is a view of it).
"""
from ..ops import ACT_GELU, ACT_NONE, ACT_RELU, ACT_TANH, KROW, KROW_GATHER, KROW_TAPS, ROWK, ROWK_GATHER  # noqa: F401
from .cnn import GridFeatBackbone, cnn_backward, cnn_backward_steps, cnn_early_split, cnn_forward  # noqa: F401
from .e2e import ClipBert, load_state_dict_with_mismatch  # noqa: F401
from .encoder import ClipBertBaseModel, encoder_backward, encoder_forward  # noqa: F401
from .heads import (ClipBertForMultipleChoice, ClipBertForPreTraining, ClipBertForRegression, ClipBertForSequenceClassification,  # noqa: F401
                    ClipBertForVideoTextRetrieval, cross_entropy_none, head_loss_none)
from .modules import (RESNET50_STAGES, BatchNorm1d, BertEmbeddings, BertEncoder, BertLayer, BertPooler, BottleneckBlock, Conv2d,  # noqa: F401
                      Embedding, FrozenBatchNorm2d, LayerNorm, Linear, VisualInputEmbedding, as_config)
from .runtime import Runtime  # noqa: F401
