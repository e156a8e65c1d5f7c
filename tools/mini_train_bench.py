"""Eager time of one DCCRNet_mini output-distillation training step
(clskd.distill_mini.OutputDistillation.train_step) at the reference's training shape, batch
cfg.batch = 32 x 3 s (segment = 3), for the three KD terms.

Per KD kind: `--runs` runs of `--steps` steps after `--warmup` warm-up steps each.  A run takes
  device_ms        stream events around the timed steps / steps (first enqueue to last kernel)
  host_enqueue_ms  host clock around the same steps before any synchronise / steps
  wall_ms          host clock including the closing synchronise / steps
and the tool prints one JSON line per kind (medians with ranges over the runs), appended to
--out.  A step whose host enqueue time reaches its device time is launch-bound: the device waits
for the host, and capture of the step is what would shorten it.

--teacher fixed (default): the frozen teacher returns a precomputed waveform, so the step is the
student's taped forward, the losses, the backward and Adam; --teacher dccrn: a clskd.DCCRN of the
teacher configuration runs in every step (the stand-in of DESIGN §7).
--cpu-ref: also time the float32 CPU step reference (tests/mini_train_ref.py, autograd through
the oracle) on this host with min(16, usable cores) threads, for context.
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
import torch.nn as nn  # noqa: E402

from clskd import config as cfg  # noqa: E402
from clskd.data import synthetic_pairs  # noqa: E402


class FixedTeacher(nn.Module):
    def __init__(self, wav):
        super().__init__()
        self.register_buffer("wav", wav)

    def forward(self, x):
        return self.wav


def _stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def build(kind, teacher, X, dev):
    from clskd.asteroid import DCCRNet_mini, load_conf
    from clskd.distill_mini import OutputDistillation
    from clskd.train import FlatAdam, FlatParams
    student = DCCRNet_mini.from_pretrained(load_conf(np.load(os.path.join(
        REPO, "tests", "golden", "asteroid_mini.npz")))).to(dev).train()
    if teacher == "dccrn":
        from clskd.model import DCCRN
        from clskd.weights import TEACHER_SEED, apply_recipe
        t = apply_recipe(DCCRN(masking_mode="E", use_clstm=True, **cfg.TEACHER), TEACHER_SEED).to(dev)
    else:
        g = torch.Generator().manual_seed(3)
        t = FixedTeacher((0.05 * torch.randn(X.shape, generator=g)).to(dev))
    kd = OutputDistillation(t, student, kd=kind)
    flat = FlatParams(kd.student)
    opt = FlatAdam(flat, lr=cfg.learning_rate, weight_decay=5e-4)
    return kd, flat, opt


def measure(kd, flat, opt, batch, steps, warmup):
    for _ in range(warmup):
        kd.train_step(batch, flat, opt)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        loss = kd.train_step(batch, flat, opt)
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return e0.elapsed_time(e1) / steps, (t1 - t0) * 1e3 / steps, (t2 - t0) * 1e3 / steps, float(loss.item())


def cpu_reference_ms(kind, B, L, reps=2):
    import mini_train_ref as M
    n = min(16, len(os.sched_getaffinity(0)))
    torch.set_num_threads(n)
    x, y, t = M.seeded_batch(B, L, seed=1)
    M.reference_step(kind, x, y, t, torch.float32)  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        M.reference_step(kind, x, y, t, torch.float32)
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=cfg.batch)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kinds", default="spkd,mse,stft")
    ap.add_argument("--teacher", choices=("fixed", "dccrn"), default="fixed")
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mini_train.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mini_train_bench: no HIP device (a CPU run gives no time)")
    dev = torch.device("cuda", 0)
    L = int(a.seconds * cfg.fs)
    noisy, clean = synthetic_pairs(a.batch, L, seed=1)
    k = 0.3 / np.abs(noisy).max()
    X, y = torch.from_numpy(noisy * k).to(dev), torch.from_numpy(clean * k).to(dev)
    for kind in a.kinds.split(","):
        kd, flat, opt = build(kind, a.teacher, X, dev)
        runs = [measure(kd, flat, opt, (X, y), a.steps, a.warmup) for _ in range(a.runs)]
        devms, host, wall = ([r[i] for r in runs] for i in range(3))
        rec = dict(bench="mini_train_step", kd=kind, teacher=a.teacher, B=a.batch, L=L, steps=a.steps,
                   warmup=a.warmup, runs=a.runs, device_ms=_stat(devms), host_enqueue_ms=_stat(host),
                   wall_ms=_stat(wall), last_loss=runs[-1][3],
                   host_over_device=round(statistics.median(host) / statistics.median(devms), 3),
                   gpu=torch.cuda.get_device_name(0))
        if a.cpu_ref:
            ms, n = cpu_reference_ms(kind, a.batch, L)
            rec.update(cpu_ref_fp32_ms=round(ms, 1), cpu_ref_threads=n)
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
