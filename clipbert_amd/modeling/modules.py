"""Parameter / buffer holders under the reference's state-dict keys, in its registration order (params.ParamBank's flat layout)."""
import math
from types import SimpleNamespace

import torch
from torch import nn

FROZEN_BN_EPS = 1e-5
RESNET50_STAGES = (("res2", 3, 64, 256, 1), ("res3", 4, 128, 512, 2), ("res4", 6, 256, 1024, 2),
                   ("res5", 3, 512, 2048, 2))


def _cfg_get(config, key, default=None):
    if isinstance(config, dict):
        return config.get(key, default)
    return getattr(config, key, default)


def as_config(config):
    """Accepts a dict (src/configs/base_model.json contents + task keys) or any attribute bag."""
    if isinstance(config, dict):
        return SimpleNamespace(**config)
    return config


class Linear(nn.Module):
    def __init__(self, in_features, out_features, std=0.02):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.randn(out_features, in_features) * std)
        self.bias = nn.Parameter(torch.zeros(out_features))


class Embedding(nn.Module):
    def __init__(self, n, dim, std=0.02, padding_idx=None):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(n, dim) * std)
        self.padding_idx = padding_idx
        if padding_idx is not None:
            with torch.no_grad():
                self.weight[padding_idx].zero_()


class LayerNorm(nn.Module):
    def __init__(self, dim, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))
        self.eps = eps


class FrozenBatchNorm2d(nn.Module):
    """detectron2.layers.FrozenBatchNorm2d: four buffers, y = x*scale + shift with fixed statistics."""
    def __init__(self, c):
        super().__init__()
        self.register_buffer("weight", torch.ones(c))
        self.register_buffer("bias", torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))


class Conv2d(nn.Module):
    """Conv weight in the reference's OIHW logical shape (channels_last memory image = KRSC) plus an
    optional FrozenBN child called ``norm`` as detectron2 names it."""
    def __init__(self, cin, cout, k, stride=1, pad=0, norm=True):
        super().__init__()
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, k, stride, pad
        w = torch.randn(cout, cin, k, k) * math.sqrt(2.0 / (cout * k * k))
        self.weight = nn.Parameter(w.contiguous(memory_format=torch.channels_last))
        self.norm = FrozenBatchNorm2d(cout) if norm else None
        self._ss = None

    def scale_shift(self):
        """fp32 per-channel (scale, shift) of the frozen affine; cached (buffers are constants)."""
        if self.norm is None:
            return None, None
        if self._ss is None or self._ss[0].device != self.norm.weight.device:
            n = self.norm
            scale = (n.weight.float() * (n.running_var.float() + FROZEN_BN_EPS).rsqrt()).contiguous()
            shift = (n.bias.float() - n.running_mean.float() * scale).contiguous()
            self._ss = (scale, shift)
        return self._ss

    def _load_from_state_dict(self, *a, **kw):
        self._ss = None
        return super()._load_from_state_dict(*a, **kw)


class BottleneckBlock(nn.Module):
    def __init__(self, cin, mid, cout, stride):
        super().__init__()
        self.shortcut = Conv2d(cin, cout, 1, stride) if cin != cout else None
        self.conv1 = Conv2d(cin, mid, 1, stride)          # stride in the 1x1 (STRIDE_IN_1X1=True)
        self.conv2 = Conv2d(mid, mid, 3, 1, 1)
        self.conv3 = Conv2d(mid, cout, 1)


class _Stem(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = Conv2d(3, 64, 7, 2, 3)


class _ResNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.stem = _Stem()
        cin = 64
        for name, n_blocks, mid, cout, stride in RESNET50_STAGES:
            blocks = []
            for b in range(n_blocks):
                blocks.append(BottleneckBlock(cin, mid, cout, stride if b == 0 else 1))
                cin = cout
            setattr(self, name, nn.ModuleList(blocks))


class _Detectron2Model(nn.Module):
    """Only ``backbone`` of the GeneralizedRCNN is ever executed by ClipBERT (grid_feat.py:95-97);
    the RPN / ROI heads of the reference checkpoint are ignored at load time."""
    def __init__(self):
        super().__init__()
        self.backbone = _ResNet()


class _GridConv(nn.Module):
    """grid_encoder[0]: conv3x3(2048 -> hidden, no bias)  (grid_feat.py:16-21,43-45)."""
    def __init__(self, cin, cout):
        super().__init__()
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, 3, 1, 1
        w = torch.randn(cout, cin, 3, 3) * math.sqrt(2.0 / (cin * 9))
        self.weight = nn.Parameter(w.contiguous(memory_format=torch.channels_last))
        self.norm = None

    def scale_shift(self):
        return None, None


class BertEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.word_embeddings = Embedding(config.vocab_size, config.hidden_size, config.initializer_range,
                                         padding_idx=_cfg_get(config, "pad_token_id", 0))
        self.position_embeddings = Embedding(config.max_position_embeddings, config.hidden_size, config.initializer_range)
        self.token_type_embeddings = Embedding(config.type_vocab_size, config.hidden_size, config.initializer_range)
        self.LayerNorm = LayerNorm(config.hidden_size, config.layer_norm_eps)


class VisualInputEmbedding(nn.Module):
    def __init__(self, config):
        super().__init__()
        r = config.initializer_range
        self.position_embeddings = Embedding(config.max_position_embeddings, config.hidden_size, r)   # unused (as in the reference)
        self.row_position_embeddings = Embedding(config.max_grid_row_position_embeddings, config.hidden_size, r)
        self.col_position_embeddings = Embedding(config.max_grid_col_position_embeddings, config.hidden_size, r)
        self.token_type_embeddings = Embedding(1, config.hidden_size, r)
        self.LayerNorm = LayerNorm(config.hidden_size, config.layer_norm_eps)


class _SelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        d = config.hidden_size
        self.query, self.key, self.value = Linear(d, d), Linear(d, d), Linear(d, d)


class _Dense(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.dense = Linear(in_features, out_features)


class _DenseLN(nn.Module):
    """``dense`` + ``LayerNorm``: attention.output, output and the prediction head's transform"""
    def __init__(self, config, in_features=None):
        super().__init__()
        self.dense = Linear(in_features or config.hidden_size, config.hidden_size)
        self.LayerNorm = LayerNorm(config.hidden_size, config.layer_norm_eps)


class _Attention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self = _SelfAttention(config)
        self.output = _DenseLN(config)


class BertLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = _Attention(config)
        self.intermediate = _Dense(config.hidden_size, config.intermediate_size)
        self.output = _DenseLN(config, config.intermediate_size)


class BertEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.layer = nn.ModuleList([BertLayer(config) for _ in range(config.num_hidden_layers)])


class BertPooler(_Dense):
    def __init__(self, config):
        super().__init__(config.hidden_size, config.hidden_size)


class BatchNorm1d(nn.Module):
    """parameter / buffer holder with torch.nn.BatchNorm1d's state-dict keys"""
    def __init__(self, d, eps=1e-5, momentum=0.1):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.bias = nn.Parameter(torch.zeros(d))
        self.register_buffer("running_mean", torch.zeros(d))
        self.register_buffer("running_var", torch.ones(d))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self.eps, self.momentum = eps, momentum


def _make_mlp(d, n_out):
    return nn.ModuleList([Linear(d, d * 2), nn.Identity(), Linear(d * 2, n_out)])


class _Decoder(nn.Module):
    def __init__(self, weight, bias):
        super().__init__()
        self.weight = weight          # tied to bert.embeddings.word_embeddings.weight
        self.bias = bias              # same Parameter as predictions.bias (transformers.py:507-510)


class _LMPredictionHead(nn.Module):
    def __init__(self, config, word_weight):
        super().__init__()
        self.transform = _DenseLN(config)
        self.bias = nn.Parameter(torch.zeros(config.vocab_size))
        self.decoder = _Decoder(word_weight, self.bias)


class _PreTrainingHeads(nn.Module):
    def __init__(self, config, word_weight):
        super().__init__()
        self.predictions = _LMPredictionHead(config, word_weight)
        self.seq_relationship = Linear(config.hidden_size, 2)
