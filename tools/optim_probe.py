"""cb_adamw against the two other algorithms of cb_optim_step (Adam, Adamax) on one flat range of 96 M elements (the size of
profiles/r03p_adamw_nt.txt): each launch between two HIP events, the three algorithms interleaved launch by launch so that clock drift
and other tenants hit them equally.  Prints and writes median / min / max per algorithm and the GB/s against the 30 bytes per element all
three must move.  The yardstick is cb_adamw IN THE SAME RUN.  One process; it ends itself after --limit seconds.

    python tools/optim_probe.py [--launches 30] [--out profiles/optim_variants.txt]"""
import argparse
import faulthandler
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from clipbert_amd import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--elements", type=int, default=96 * 1024 * 1024 + 7)
ap.add_argument("--limit", type=int, default=240, help="seconds after which the process ends itself")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "optim_variants.txt"))
args = ap.parse_args()
assert args.launches >= 20
faulthandler.dump_traceback_later(args.limit, exit=True)
assert torch.cuda.is_available(), "optim_probe needs the GPU: a host timing says nothing about it"

dev = torch.device("cuda", 0)
n = args.elements
p, g, m = (torch.randn(n, device=dev) * 0.01 for _ in range(3))
second = {name: (torch.randn(n, device=dev) * 0.01).abs_() for name in ("adamw", "adam", "adamax")}
w16 = torch.empty(n, dtype=torch.bfloat16, device=dev)
sq = torch.tensor([4.0], device=dev)


def hyper(eps):
    return torch.tensor(ops.adamw_hyper(1e-4, 0.9, 0.98, eps, 1e-3, 10, 5.0, 1.0), dtype=torch.float32, device=dev)


hp6, hp8 = hyper(1e-6), hyper(1e-8)
runs = {"adamw": lambda: ops.adamw(p, g, m, second["adamw"], w16, hp6, sq),
        "adam": lambda: ops.optim_step(_lib.OPT_ADAM, p, g, m, second["adam"], w16, hp8, sq),
        "adamax": lambda: ops.optim_step(_lib.OPT_ADAMAX, p, g, m, second["adamax"], w16, hp8, sq)}
for _ in range(args.warmup):
    for fn in runs.values():
        fn()
torch.cuda.synchronize()
events = {name: [] for name in runs}
for _ in range(args.launches):
    for name, fn in runs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        events[name].append((e0, e1))
torch.cuda.synchronize()
assert bool(torch.isfinite(p).all())
lines = [f"{n} elements, {args.launches} timed launches per algorithm after {args.warmup} warm-up rounds, interleaved adamw / adam / adamax; "
         f"HIP events around each launch; {torch.cuda.get_device_name(0)}"]
stats = {}
for name, evs in events.items():
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
    stats[name] = (statistics.median(us), us[0], us[-1])
    med = stats[name][0]
    lines.append(f"{'cb_adamw' if name == 'adamw' else 'cb_optim_step ' + name:22s} median {med:7.1f} us  min {us[0]:7.1f}  max {us[-1]:7.1f}   "
                 f"{n * 30 / med / 1e3:6.0f} GB/s at the median")
_med, lo, hi = stats["adamw"]
for name in ("adam", "adamax"):
    med = stats[name][0]
    where = "inside" if lo <= med <= hi else "OUTSIDE"
    lines.append(f"{name}: median {med:.1f} us is {where} cb_adamw's own spread [{lo:.1f}, {hi:.1f}] us ({med / stats['adamw'][0]:.3f} x its median)")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
