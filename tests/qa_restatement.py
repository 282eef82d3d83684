"""float64 restatement of the video-QA validation arithmetic (src/tasks/run_video_qa.py:261-279 and the loss accumulated at :250-259) on a
(n_clips, n_q, C) stack of per-clip logits: pool over the clips, arg-max over the classes or round-and-clamp of the count regression,
and per question the mean over the clips of the per-clip loss.  Test infrastructure only: plain torch on the CPU, shared by
test_qa_predict.py and test_qa_loop.py.

The bounds below follow the kernel's own order of operations (clipbert_amd/csrc/qa.hip, clip_pool.h); none of them comes from a run of it.
eps = 2^-24 is the fp32 unit round-off, X = max|x| over the stack.

pooled_bound = 4 eps (n_clips + 2) max(1, X).  First order, a pooled logit carries at most (n_clips + 2) eps X: the n_clips - 1 additions
and the division of the mean; nothing for the maximum; for the max-shifted log-sum-exp the shift, the exponentials, their n_clips - 1
additions, the logarithm and the final addition, each term's error entering the logarithm weighted by its share of the sum.  This is the
per-logit figure of mc_restatement.score_bound (cb_mc_predict pools with the same code); the 4 is the margin.

loss_bound (classify) = 4 eps [(5 + 2 n_clips) X + A + 2 + (4 + n_clips) ln C], A = ceil(C / lanes) + log2(lanes), lanes = 64 for C <= 64
(one wave per question, 6 shuffle levels) and 256 above (a plain sum of ceil(C / 256) terms per lane, 6 shuffle levels, 2 levels over the
four waves).  Per clip, lse = m + log S with S = sum_c exp(x_c - m) in [1, C] and m the exact maximum:
  the shifts x_c - m round by eps |x_c - m| <= 2 eps X each, which the logarithm sees weighted by the terms' shares: 2 eps X;
  expf costs a relative 2 eps per term (a few ulps, weighted likewise): 2 eps;
  the A additions cost a relative A eps in S, A eps in log S;
  logf costs 2 eps ln C; the addition m + log S costs eps (X + ln C); subtracting x[label] costs eps (2 X + ln C).
That is eps [5 X + A + 2 + 4 ln C] per clip, each per-clip loss being at most 2 X + ln C.  The n_clips - 1 additions over the clips and the
division cost n_clips eps (2 X + ln C) on the mean.  The sum and a 4x margin give the figure.

count_loss_bound = 4 eps (n_clips + 3) D^2, D = max|x - label|: the difference costs a relative eps, its square 3 eps in all, the
n_clips - 1 additions and the division n_clips eps; 4x margin."""
import math

import torch

EPS = 2.0 ** -24                                            # fp32 unit round-off
SMALL_C = 64                                                # up to here the kernel runs one wave per question


def pool(stack: torch.Tensor, method: str) -> torch.Tensor:
    """float64 (n_q, C): :262-271"""
    x = stack.detach().cpu().double()
    assert x.dim() == 3, tuple(x.shape)
    if method == "mean":
        return x.mean(0)
    if method == "max":
        return x.max(0)[0]
    if method == "lse":
        return torch.logsumexp(x, dim=0)
    raise ValueError(method)


def classify(stack: torch.Tensor, method: str, labels=None):
    """-> (pooled float64 (n_q, C), pred int64 (n_q,), loss float64 (n_q,) | None).  torch.max: the lowest index among equal maxima, a NaN
    above every number.  loss[q] = mean over the clips of cross_entropy(x[k, q, :], labels[q]) (:250-259)."""
    pooled = pool(stack, method)
    loss = None
    if labels is not None:
        x = stack.detach().cpu().double()
        lab = torch.as_tensor(labels).long().view(1, -1, 1).expand(x.shape[0], -1, 1)
        loss = (torch.logsumexp(x, dim=2) - x.gather(2, lab)[..., 0]).mean(0)
    return pooled, pooled.max(dim=-1)[1], loss


def count(stack: torch.Tensor, method: str, labels=None):
    """-> (pooled float64 (n_q, 1), pred int64 (n_q,), loss float64 (n_q,) | None): :278, and the mean over the clips of (x - label)^2"""
    pooled = pool(stack, method)
    assert pooled.shape[1] == 1
    loss = None
    if labels is not None:
        x = stack.detach().cpu().double()[..., 0]
        loss = ((x - torch.as_tensor(labels).double().view(1, -1)) ** 2).mean(0)
    return pooled, (pooled + 0.5).long().clamp(min=1, max=10).view(-1), loss


def pooled_bound(stack: torch.Tensor) -> float:
    return 4.0 * EPS * (stack.shape[0] + 2) * max(1.0, float(stack.detach().abs().max()))


def loss_bound(stack: torch.Tensor) -> float:
    n_clips, _, c = stack.shape
    lanes = 64 if c <= SMALL_C else 256
    adds = math.ceil(c / lanes) + math.log2(lanes)
    big = float(stack.detach().abs().max())
    return 4.0 * EPS * ((5 + 2 * n_clips) * big + adds + 2 + (4 + n_clips) * math.log(c))


def count_loss_bound(stack: torch.Tensor, labels: torch.Tensor) -> float:
    d = float((stack.detach().double()[..., 0] - torch.as_tensor(labels).double().view(1, -1)).abs().max())
    return 4.0 * EPS * (stack.shape[0] + 3) * d * d


def top2_margin(pooled: torch.Tensor) -> torch.Tensor:
    """float64 (n_q,): best minus second-best pooled logit of every question (inf for a single class)"""
    p = pooled.double()
    if p.shape[1] == 1:
        return torch.full((p.shape[0],), float("inf"), dtype=torch.float64)
    top = p.topk(2, dim=1)[0]
    return top[:, 0] - top[:, 1]


def round_distance(pooled: torch.Tensor) -> torch.Tensor:
    """float64 (n_q,): the distance of pooled + 0.5 to the nearest integer -- the count answer is decided when it exceeds the pooled bound"""
    t = pooled.double().view(-1) + 0.5
    return (t - t.round()).abs()
