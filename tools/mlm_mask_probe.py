"""What one cb_mlm_mask launch costs on the GPU: a hipGraph of N launches over one (rows, Lt) id matrix, replayed between HIP events.

    python tools/mlm_mask_probe.py [--rows 32] [--lt 30] [--launches 100] [--replays 200] [--windows 5] [--out FILE.json]

Prints one JSON line: microseconds per launch inside the graph, median / min / max over the windows, for the given shape and for a
64 x as large one (where the kernel, not the launch, is what is timed).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipbert_amd import ops                                  # noqa: E402
from clipbert_amd.modeling.runtime import _SITE_MLM, _seed    # noqa: E402


def per_launch_us(rows, lt, launches, replays, windows, dev):
    g = torch.Generator().manual_seed(rows * 1000 + lt)
    ids = torch.randint(1000, 30522, (rows, lt), generator=g, dtype=torch.int64)
    ids[:, 0], ids[:, -1] = 101, 102
    ids = ids.to(dev)
    out, lab = torch.empty_like(ids), torch.empty_like(ids)
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    seed = _seed(_SITE_MLM, 0, 0)

    def body():
        for _ in range(launches):
            ops.mlm_mask(ids, 0.15, seed, word, vocab_size=30522, out_ids=out, out_labels=lab)
        ops.counter_add(word)

    body()                                                    # warm: code object loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(replays):
            graph.replay()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1000.0 / (replays * (launches + 1)))      # (+ 1: the counter launch, a launch like these)
    labelled = int((lab != -100).sum().item())
    return dict(rows=rows, lt=lt, us_median=round(statistics.median(times), 3), us_min=round(min(times), 3), us_max=round(max(times), 3),
                labelled_last=labelled)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--lt", type=int, default=30)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlm_mask_probe needs a GPU")
    dev = torch.device("cuda", 0)
    res = dict(probe="mlm_mask", launches=a.launches, replays=a.replays, windows=a.windows,
               shapes=[per_launch_us(a.rows, a.lt, a.launches, a.replays, a.windows, dev),
                       per_launch_us(a.rows * 64, a.lt, a.launches, a.replays, a.windows, dev)])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
