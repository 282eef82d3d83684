#!/usr/bin/env python
"""cb_gemm_plan / cb_gemm_workspace_bytes of the built library against another build of it (a variant made by
`python -m clipbert_amd.build --variant NAME --csrc <csrc of another commit>`): return code, the four plan words, the scratch size and,
on refusal, the error text must be equal for every call of one corpus.  Host logic only: nothing is launched, no GPU is needed.

    python tools/plan_equiv.py [--variant parent] [--random 24000] [--seed 1]

The corpus: every key of csrc/gemm_tuned.h; every problem of the sweeps behind the launch-cost model (profiles/r03m_gemm_model_fit.json);
a seeded random sample over what the dispatcher branches on.  Prints how many calls took each kernel structure, so that a corpus that
misses a branch is visible; exit status 1 if any call differs."""
import argparse
import collections
import ctypes as C
import json
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fit_gemm_model as F  # noqa: E402
from clipbert_amd import _lib, build  # noqa: E402

PTR = 1 << 20                                              # (aligned dummy: nothing is dereferenced)


def desc(dtype=1, M=256, N=256, K=256, a_mode=0, b_mode=0, taps=1, batch=1, **kw):
    """a descriptor whose leading dimensions, tables and conv geometry fit its modes; kw overrides any field afterwards"""
    d = _lib.GemmDesc()
    C.memset(C.byref(d), 0, C.sizeof(d))
    d.dtype, d.M, d.N, d.K, d.a_mode, d.b_mode, d.batch = dtype, M, N, K, a_mode, b_mode, batch
    d.A = d.B = d.C = PTR
    d.a_bytes = d.b_bytes = 1 << 30
    d.lda = M if a_mode == 2 else K
    d.ldb = {0: K, 2: N, 3: N * taps, 4: 0}.get(b_mode, K)
    d.ldc = N
    if a_mode == 1 or b_mode in (3, 4):
        d.R, d.S = (3, 3) if taps == 9 else (taps, 1)
        d.Cin = (N if b_mode == 4 else K) // taps
        d.H = d.W = 8
        d.sW, d.sH = d.Cin, 8 * d.Cin
        d.a_tab = PTR if a_mode == 1 else 0
        d.b_tab = PTR if b_mode == 4 else 0
    if batch > 1:
        d.batch_stride_a, d.batch_stride_b, d.batch_stride_c = K * M, K * N, M * N
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def corpus(n_random, seed):
    tuned = open(os.path.join(ROOT, "clipbert_amd", "csrc", "gemm_tuned.h")).read()
    ws = dict(splitk_ws=PTR, splitk_ws_bytes=128 << 20)
    for m in re.finditer(r"^\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), ", tuned, re.M):
        a, b, M, N, K, batch, taps, split = map(int, m.groups())
        wg = dict(c_f32=1, accumulate=1) if a == 2 else {}
        for table in (0, 1):
            yield table, desc(1, M, N, K, a, b, taps, batch, split_k=split, **wg, **ws)
            yield table, desc(1, M, N, K, a, b, taps, batch, split_k=split, **wg)
    fit = json.load(open(os.path.join(ROOT, "profiles", "r03m_gemm_model_fit.json")))
    for p in F.load([os.path.join(ROOT, s) for s in fit["sweeps"]]):
        wg = dict(c_f32=1, accumulate=1) if p["form"] == "wgrad" else {}
        for table in (0, 1):
            yield table, desc(1, p["M"], p["N"], p["K"], p["a_mode"], p["b_mode"], p["taps"], p["batch"], split_k=p["split_k"], **wg, **ws)
    rng = random.Random(seed)
    some = lambda prob: rng.random() < prob                                                                 # noqa: E731
    for _ in range(n_random):
        a_mode, b_mode = rng.choice([(0, 0)] * 4 + [(0, 2)] * 3 + [(2, 2)] * 4 + [(1, 0), (1, 3), (0, 3), (2, 4)] * 2 +
                                    [(0, 4), (1, 2), (1, 4), (2, 0), (2, 3)] + ([(3, 0), (0, 5)] if some(0.1) else []))
        taps = rng.choice([1, 9]) if (a_mode == 1 or b_mode in (3, 4)) else 1
        M = rng.choice([1, 4, 63, 64, 72, 200, 256, 777, 1312, 2624, 5000, 12544, 40000, 50176, 131072, 200704])
        N = rng.choice([8, 72, 1000] if b_mode == 4 else [1, 2, 8, 64, 72, 128, 256, 512, 768, 1000, 1024, 2304, 3072, 18432])
        K = rng.choice([8, 64, 72, 128, 256, 512, 768, 2304, 4608, 18432, 100352])
        if some(0.06):                                                  # the regime of the streaming structure: short reduction, many rows
            M, N, K = rng.choice([40000, 50176, 131072, 200704]), rng.choice([128, 256, 512]), rng.choice([64, 128])
        if some(0.02):
            M, N = rng.choice([(0, N), (M, 0)])
        if taps == 9:                                                   # (mostly consistent with the mode's K / N = taps x Cin contract)
            if b_mode == 4:
                N = 9 * rng.choice([8, 64, 128, 100])
            else:
                K = 9 * rng.choice([8, 64, 128, 100])
        wgrad = a_mode == 2 and some(0.8)
        kw = dict(tile=rng.choice([0, 0, 0, 0] + list(range(10))) if some(0.5) else 0, split_k=rng.choice([0, 1, 1, 2, 3, 4, 8, 64]) if some(0.4 if wgrad else 0.12) else 1,
                  schedule=rng.choice([0, 0, 1, 2, 3, 4]), xcd_order=rng.choice([0, 0, 1, 2]), c_f32=int(wgrad or some(0.1)),
                  accumulate=rng.choice([1, 1, 0, 2]) if wgrad else rng.choice([0, 0, 0, 1, 2]))
        r = rng.random()                                                # scratch: present / absent / too small / misaligned
        if r < 0.55:
            kw.update(splitk_ws=PTR, splitk_ws_bytes=128 << 20)
        elif r < 0.7:
            kw.update(splitk_ws=PTR, splitk_ws_bytes=rng.choice([4096, 65536, 1 << 20, 8 << 20]))
        elif r < 0.8:
            kw.update(splitk_ws=PTR + 4, splitk_ws_bytes=128 << 20)
        for field, ld, prob in (("C2", "ldc2", 0.06), ("residual", "ldr", 0.08), ("mask", "ldm", 0.06), ("gelu_grad_pre", "ld_gelu", 0.05)):
            if some(prob):
                kw[field], kw[ld] = PTR + (2 if some(0.1) else 0), N + (1 if some(0.1) else 0)
        if "mask" in kw and "gelu_grad_pre" in kw:                        # (refused together since the widths of the epilogue became one function)
            del kw["gelu_grad_pre"], kw["ld_gelu"]
        plain_wgrad = (a_mode, b_mode) == (2, 2)                          # (row sums / norm shares: mostly where gemm_prepare admits them)
        for field, prob in (("shift", 0.15), ("scale", 0.1), ("a_rowsum", 0.15 if plain_wgrad else 0.01), ("c_rowmap", 0.03),
                            ("sq_slots", 0.25 if wgrad and kw["accumulate"] != 1 else 0.01)):
            if some(prob):
                kw[field] = PTR
        if "sq_slots" in kw:
            kw["sq_slots_n"] = rng.choice([1 << 30, 1 << 30, 1])
        if some(0.1):
            kw["act"] = rng.choice([1, 2, 4, 5])
        if some(0.05):
            kw["relu_after"] = 1
        if some(0.05):
            kw["dropout_p"] = 0.1
        if some(0.04):
            kw.update(relu_bwd=1, mask=kw.get("mask", PTR), ldm=kw.get("ldm", N), post_scale=PTR if some(0.7) else 0)
        if some(0.03):
            kw.update(zero_fill_pitch=rng.choice([8, -1]))
        if some(0.05):
            kw["alpha"] = 0.5
        d = desc(rng.choice([1, 1, 1, 1, 0]), M, N, K, a_mode, b_mode, taps, rng.choice([2, 12]) if some(0.08) else 1, **kw)
        if some(0.05):                                                  # unaligned leading dimensions and pointers
            d.lda += 1
        if some(0.05):
            d.ldb += 1
        if some(0.05):
            d.ldc += rng.choice([1, 4])
        if some(0.03):
            d.A += 2
        if some(0.03):
            d.C += rng.choice([2, 8])
        yield int(some(0.6)), d


def ask(lib, table, d):
    out, nbytes = (C.c_int32 * 4)(), C.c_int64(0)
    rc = lib.cb_gemm_plan(C.byref(d), table, out)
    err = lib.cb_last_error().decode(errors="replace") if rc else ""
    rc2 = lib.cb_gemm_workspace_bytes(C.byref(d), C.byref(nbytes))
    err2 = lib.cb_last_error().decode(errors="replace") if rc2 else ""
    return (rc, tuple(out), err, rc2, nbytes.value, err2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="parent")
    ap.add_argument("--random", type=int, default=24000)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    new, old = _lib.load(), _lib.load(build.variant_path(args.variant))
    took, refusals, differ = collections.Counter(), collections.Counter(), 0
    for table, d in corpus(args.random, args.seed):
        got, want = ask(new, table, d), ask(old, table, d)
        tile = got[1][0]
        took["refused" if got[0] else "empty (M or N zero)" if tile == 0 else "4-wave" if tile <= 4 else "8-wave" if tile <= 7 else
             "streaming" if tile == 8 else "few rows"] += 1
        took["8-wave with a slab split"] += int(got[0] == 0 and 5 <= tile <= 7 and got[1][1] > 1)
        took["4-wave with a K split"] += int(got[0] == 0 and 1 <= tile <= 4 and got[1][1] > 1)
        if got[0]:
            refusals[re.sub(r"-?\d+", "#", got[2])[:70]] += 1
        if got != want:
            differ += 1
            if differ <= 10:
                print("DIFFERS:", {f: getattr(d, f) for f, _ in d._fields_ if getattr(d, f)}, "table", table, "\n  new", got, "\n  old", want)
    print(json.dumps(dict(calls=sum(v for k, v in took.items() if " with " not in k), took=dict(took), refusals=dict(refusals), differ=differ), indent=1))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
