"""Eager time of one supervised training step (clskd.supervised.SupervisedTraining.train_step) at
the reference's training shape, batch cfg.batch = 32 x 3 s, for the student clskd.DCCRN and the
fixture DCCRNet_mini, and the isolated time and achieved GB/s of each kernel of csrc/sup_loss.hip
at that size, with clskd_mse_loss_grad on the same n as the yardstick of the MSE path.

Step records (one JSON line per model and mode): `--runs` runs of `--steps` steps after `--warmup`
warm-up steps each;
  device_ms        stream events around the timed steps / steps
  host_enqueue_ms  host clock around the same steps before any synchronise / steps
  wall_ms          host clock including the closing synchronise / steps
as medians with ranges over the runs.  Kernel records: stream events around `--kreps` back-to-back
calls / kreps, the median over `--runs` runs, and bytes / time for the bytes the entry moves at
least once (DESIGN.md lists them).  Appended to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "speech-enhancement-clskd_amd"), os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from clskd import config as cfg  # noqa: E402


def _stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def build(model, mode, dev):
    from clskd.supervised import SupervisedTraining
    from clskd.train import FlatAdam, FlatParams
    if model == "mini":
        from clskd.asteroid import DCCRNet_mini, load_conf
        m = DCCRNet_mini.from_pretrained(load_conf(np.load(os.path.join(
            REPO, "tests", "golden", "asteroid_mini.npz")))).to(dev).train()
    else:
        from clskd.model import DCCRN
        from clskd.weights import STUDENT_SEED, apply_recipe
        m = apply_recipe(DCCRN(masking_mode="E", use_clstm=True, **cfg.STUDENT), STUDENT_SEED).to(dev).train()
    mod = SupervisedTraining(m, mode)
    flat = FlatParams(mod.student)
    return mod, flat, FlatAdam(flat, lr=cfg.learning_rate)


def measure(mod, flat, opt, batch, steps, warmup):
    for _ in range(warmup):
        mod.train_step(batch, flat, opt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        loss = mod.train_step(batch, flat, opt)
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return e0.elapsed_time(e1) / steps, (t1 - t0) * 1e3 / steps, (t2 - t0) * 1e3 / steps, float(loss.item())


def time_call(fn, reps, runs):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def kernel_records(B, L, reps, runs, dev):
    """Each entry alone, on buffers of the step's size, workspaces allocated outside the timed
    region (raw library calls: the timed region is launches only)."""
    from clskd import ops
    lib, ptr, st = ops.lib(), ops.ptr, ops._stream
    import ctypes as C
    g = torch.Generator().manual_seed(1)
    s = (0.1 * torch.randn(B, L, generator=g)).to(dev)
    y = (0.1 * torch.randn(B, L, generator=g)).to(dev)
    d = torch.zeros(B, L, device=dev)
    T = cfg.n_frames(L)
    clean = torch.randn(B, T, 514, generator=g).to(dev)
    est = torch.randn(B, T, 516, generator=g).to(dev)
    dest = torch.zeros(B, T, 516, device=dev)
    n = B * L
    work = torch.empty(int(lib.clskd_wave_loss_workspace(B, L)), dtype=torch.float64, device=dev)
    mwork = torch.empty(int(lib.clskd_mel_loss_workspace(B, T)), dtype=torch.float64, device=dev)
    swork = torch.empty(int(lib.clskd_mse_loss_grad_workspace(n)), dtype=torch.float64, device=dev)
    out, coef = torch.empty(6, device=dev), torch.empty(B, 2, device=dev)
    out2, lo = torch.empty(2, device=dev), torch.empty(1, device=dev)
    tab = ops.mel_table(dev)
    w5 = (C.c_float * 5)(1, 0, 0, 0, 0)
    spec_b = B * T * 514 * 4
    calls = {
        "wave_loss (sums + finalize)": (lambda: ops.check(lib.clskd_wave_loss(
            ptr(s), L, ptr(y), L, B, L, w5, 1.0, ptr(work), ptr(out), ptr(coef), st())), 2 * n * 4),
        "wave_loss_grad": (lambda: ops.check(lib.clskd_wave_loss_grad(
            ptr(s), L, ptr(y), L, B, L, ptr(coef), ptr(d), L, 0, st())), 3 * n * 4),
        "mse path: wave_loss + wave_loss_grad": (lambda: (
            ops.check(lib.clskd_wave_loss(ptr(s), L, ptr(y), L, B, L, w5, 1.0, ptr(work), ptr(out),
                                          ptr(coef), st())),
            ops.check(lib.clskd_wave_loss_grad(ptr(s), L, ptr(y), L, B, L, ptr(coef), ptr(d), L, 0,
                                               st()))), 5 * n * 4),
        "mse_loss_grad (yardstick)": (lambda: ops.check(lib.clskd_mse_loss_grad(
            ptr(s), ptr(y), n, 1.0, ptr(swork), ptr(lo), ptr(d), 0, st())), 3 * n * 4),
        "mel_loss (fwd + finalize)": (lambda: ops.check(lib.clskd_mel_loss(
            ptr(clean), 514, ptr(est), 516, B, T, ptr(tab), ptr(mwork), 1.0, 0, ptr(out2), st())),
            2 * spec_b),
        "mel_loss_bwd (write)": (lambda: ops.check(lib.clskd_mel_loss_bwd(
            ptr(clean), 514, ptr(est), 516, B, T, ptr(tab), 1.0, ptr(dest), 516, 0, st())),
            4 * spec_b),
    }
    recs = []
    for name, (fn, nbytes) in calls.items():
        ms = time_call(fn, reps, runs)
        med = statistics.median(ms)
        recs.append(dict(bench="sup_loss_kernel", kernel=name, B=B, L=L, T=T, reps=reps, runs=runs,
                         ms=_stat(ms), bytes=nbytes, gbps=round(nbytes / med / 1e6, 1),
                         gpu=torch.cuda.get_device_name(0)))
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=cfg.batch)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kreps", type=int, default=50)
    ap.add_argument("--dccrn-modes", default="MSE,SI-SNR,SI-SNR+LMS,MRSTFT")
    ap.add_argument("--mini-modes", default="MSE,SI-SNR,MRSTFT")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sup_train.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sup_train_bench: no HIP device (a CPU run gives no time)")
    dev = torch.device("cuda", 0)
    L = int(a.seconds * cfg.fs)
    import sup_loss_ref as S
    x, y = S.seeded_batch(a.batch, L, seed=1)
    batch = (x.to(dev), y.to(dev))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    for rec in kernel_records(a.batch, L, a.kreps, a.runs, dev):
        emit(rec)
    for model, modes in (("dccrn_student", a.dccrn_modes), ("mini", a.mini_modes)):
        for mode in [m for m in modes.split(",") if m]:
            mod, flat, opt = build("mini" if model == "mini" else "dccrn", mode, dev)
            runs = [measure(mod, flat, opt, batch, a.steps, a.warmup) for _ in range(a.runs)]
            devms, host, wall = ([r[i] for r in runs] for i in range(3))
            emit(dict(bench="sup_train_step", model=model, loss_mode=mode, B=a.batch, L=L,
                      steps=a.steps, warmup=a.warmup, runs=a.runs, device_ms=_stat(devms),
                      host_enqueue_ms=_stat(host), wall_ms=_stat(wall), last_loss=runs[-1][3],
                      host_over_device=round(statistics.median(host) / statistics.median(devms), 3),
                      gpu=torch.cuda.get_device_name(0)))


if __name__ == "__main__":
    main()
