"""float64 restatement of the scoring of the MSRVTT multiple-choice test (src/tasks/run_msrvtt_mc.py:178-195) on a (n_clips, R, C) stack
of per-clip logits: pool over the clips, softmax[:, 1] (C == 2) or sigmoid (C == 1), arg-max over each group of n_options rows.  Test
infrastructure only: plain torch on the CPU, shared by test_mc_predict.py and test_mc_loop.py."""
import torch

EPS = 2.0 ** -24                                            # fp32 unit round-off


def mc_scores(stack: torch.Tensor, n_options: int, pool: str):
    """-> (scores float64 (R,), pred int64 (R / n_options,)).  torch.max: the lowest index among equal maxima, a NaN above every number."""
    x = stack.detach().cpu().double()
    assert x.dim() == 3 and x.shape[2] in (1, 2) and x.shape[1] % n_options == 0, tuple(x.shape)
    if pool == "mean":
        pooled = x.mean(0)
    elif pool == "max":
        pooled = x.max(0)[0]
    elif pool == "lse":
        pooled = torch.logsumexp(x, dim=0)
    else:
        raise ValueError(pool)
    scores = torch.softmax(pooled, dim=1)[:, 1] if x.shape[2] == 2 else torch.sigmoid(pooled[:, 0])
    return scores, scores.view(-1, n_options).max(1)[1]


def score_bound(stack: torch.Tensor) -> float:
    """|fp32 kernel score - float64 score| <= 2 eps (n_clips + 2) max(1, max|x|) + 16 eps, eps = 2^-24.

    A pooled logit carries at most (n_clips + 2) eps max|x|: n_clips - 1 additions and a division (mean); nothing (max); or the shift by
    the maximum, the exponentials, their n_clips - 1 additions, the logarithm and the final addition (lse: each term's error enters the
    logarithm weighted by its share of the sum).  The difference of the two pooled logits of a C == 2 row doubles that.  The sigmoid has a
    slope of at most 1/4 and costs a few ulps of a number <= 1 itself (one exponential, one addition, one division); its own error and a 4x
    margin on the whole are the 16 eps and the factor in front."""
    n_clips = stack.shape[0]
    return 2.0 * EPS * (n_clips + 2) * max(1.0, float(stack.detach().abs().max())) + 16.0 * EPS


def top2_margin(scores: torch.Tensor, n_options: int) -> torch.Tensor:
    """float64 (n_q,): best minus second-best score of every group (inf for a single option)"""
    g = scores.double().view(-1, n_options)
    if n_options == 1:
        return torch.full((g.shape[0],), float("inf"), dtype=torch.float64)
    top = g.topk(2, dim=1)[0]
    return top[:, 0] - top[:, 1]
