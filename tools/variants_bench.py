"""The DCCRN variants on the device: the isolated time and achieved GB/s of the masking mode 'C' /
'R' entries (clskd_mask_cr, clskd_mask_cr_bwd) next to clskd_mask_e / clskd_mask_e_bwd on the same
buffers at the reference's training shape (batch cfg.batch = 32 x 3 s), alternated run by run in
the same process; and the eager time of one SupervisedTraining.train_step ('SI-SNR') for
(E, complex LSTM), (R, complex LSTM), (E, real LSTM) and (C, real LSTM), alternated the same way.

Kernel records: stream events around `--kreps` back-to-back calls / kreps, `--runs` runs, medians
with ranges; bytes = what the entry moves at least once (forward: spectrum and mask read, estimate
written; backward: spectrum and d est read, d mask written, and for 'E' the mask read as well);
ratio = the 'C' / 'R' median over the 'E' median, spread = the 'E' entry's (max - min) / median.
Step records as tools/sup_train_bench.py.  Appended to --out.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "speech-enhancement-clskd_amd"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "tools")]
import torch  # noqa: E402

from clskd import config as cfg  # noqa: E402

STEP_VARIANTS = (("E", True), ("R", True), ("E", False), ("C", False))


def _stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def time_group(fns, reps, runs):
    """Event time per call of every function of `fns`, alternated run by run."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(runs):
        for f, ms in zip(fns, out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
    return out


def kernel_records(B, T, reps, runs, dev):
    from clskd import ops
    g = torch.Generator().manual_seed(3)
    spec = torch.randn(B, T, 514, generator=g).to(dev)
    mask = torch.randn(B, 256, T + 1, 2, generator=g).to(dev)
    dest = torch.randn(B, T, 516, generator=g).to(dev)
    est = torch.empty(B, T, 516, device=dev)
    dmask = torch.empty_like(mask)
    n_spec, n_mask, n_est = B * T * 514 * 4, mask.numel() * 4, B * T * 516 * 4
    modes = ("E", "C", "R")
    recs = []
    for kind, fns, nbytes in (
            ("forward", [lambda m=m: ops.mask(m, spec, mask, T, est) for m in modes],
             {m: n_spec + n_mask + n_est for m in modes}),
            ("backward", [lambda m=m: ops.mask_bwd(m, spec, mask, T, dest, dmask) for m in modes],
             {m: n_spec + n_est + n_mask + (n_mask if m == "E" else 0) for m in modes})):
        ms = dict(zip(modes, time_group(fns, reps, runs)))
        med = {m: statistics.median(v) for m, v in ms.items()}
        for m in ("C", "R"):
            recs.append(dict(bench="mask_kernel", kind=kind, mode=m, B=B, T=T, reps=reps, runs=runs,
                             bytes=nbytes[m], ms=_stat(ms[m]), e_ms=_stat(ms["E"]),
                             gbps=round(nbytes[m] / med[m] / 1e6, 1),
                             e_gbps=round(nbytes["E"] / med["E"] / 1e6, 1),
                             ratio=round(med[m] / med["E"], 3),
                             e_spread=round((max(ms["E"]) - min(ms["E"])) / med["E"], 3),
                             spread=round((max(ms[m]) - min(ms[m])) / med[m], 3),
                             gpu=torch.cuda.get_device_name(0)))
    return recs


def build(variant, mode, dev):
    from clskd.model import DCCRN
    from clskd.supervised import SupervisedTraining
    from clskd.train import FlatAdam, FlatParams
    from clskd.weights import STUDENT_SEED, apply_recipe
    m = apply_recipe(DCCRN(masking_mode=variant[0], use_clstm=variant[1], **cfg.STUDENT),
                     STUDENT_SEED).to(dev).train()
    mod = SupervisedTraining(m, mode)
    flat = FlatParams(mod.student)
    return mod, flat, FlatAdam(flat, lr=cfg.learning_rate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=cfg.batch)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=20)
    ap.add_argument("--mode", default="SI-SNR")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "variants.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("variants_bench: no HIP device (a CPU run gives no time)")
    dev = torch.device("cuda", 0)
    L = int(a.seconds * cfg.fs)
    T = cfg.n_frames(L)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    for rec in kernel_records(a.batch, T, a.kreps, a.runs, dev):
        emit(rec)

    import sup_loss_ref as S
    from sup_train_bench import measure
    x, y = S.seeded_batch(a.batch, L, seed=1)
    batch = (x.to(dev), y.to(dev))
    mods = {v: build(v, a.mode, dev) for v in STEP_VARIANTS}
    runs = {v: [] for v in STEP_VARIANTS}
    for _ in range(a.runs):
        for v in STEP_VARIANTS:  # alternated
            runs[v].append(measure(*mods[v], batch, a.steps, a.warmup))
    base = None
    for v in STEP_VARIANTS:
        devms, host, wall = ([r[i] for r in runs[v]] for i in range(3))
        med = statistics.median(devms)
        base = med if base is None else base
        emit(dict(bench="variant_train_step", masking_mode=v[0], use_clstm=v[1], loss_mode=a.mode,
                  B=a.batch, L=L, steps=a.steps, warmup=a.warmup, runs=a.runs, device_ms=_stat(devms),
                  host_enqueue_ms=_stat(host), wall_ms=_stat(wall), last_loss=runs[v][-1][3],
                  spread=round((max(devms) - min(devms)) / med, 3),
                  over_e_clstm_device=round(med / base, 3), gpu=torch.cuda.get_device_name(0)))


if __name__ == "__main__":
    main()
