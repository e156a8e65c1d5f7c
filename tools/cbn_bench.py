"""ComplexBatchNorm against BatchNorm on the device: the isolated time and achieved GB/s of each
entry of csrc/cbn.hip on the student's largest activations at the reference's training shape
(batch cfg.batch = 32 x 3 s: encoder 0's output and the last normalised decoder layer's), each
next to its BatchNorm counterpart (clskd_bn_stats_partial, clskd_bn_finalize, clskd_bn_apply,
clskd_bn_bwd) on the same tensor, alternated run by run in the same process; and the eager time of
one SupervisedTraining.train_step for use_cbn=True and use_cbn=False, alternated the same way.

Kernel records: stream events around `--kreps` back-to-back calls / kreps (raw library calls,
workspaces allocated outside the timed region), `--runs` runs, medians with ranges; bytes = what the
entry moves at least once (x read by a statistics pass; x read and y written by an apply; x and dy
read twice and dx written by a backward); ratio = CBN median / BatchNorm median, and spread = the
BatchNorm counterpart's (max - min) / median over its runs.  Step records as
tools/sup_train_bench.py.  Appended to --out.
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


def _stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def time_pair(fa, fb, reps, runs):
    """Event time per call of fa and of fb, alternated: run k times fa, then fb."""
    for f in (fa, fb):
        f()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(runs):
        for f, ms in zip((fa, fb), out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
    return out


def kernel_records(name, shape, reps, runs, dev):
    from types import SimpleNamespace

    from clskd import ops
    from clskd.weights import recipe_state_dict
    lib, ptr, st, chk = ops.lib(), ops.ptr, ops._stream, ops.check
    Cn = shape[-1]
    Cc = Cn // 2
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g).to(dev)
    dy = torch.randn(*shape, generator=g).to(dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    rows = x.numel() // Cn
    n4 = x.numel() * 4
    leaves = ("Wrr", "Wri", "Wii", "Br", "Bi", "RMr", "RMi", "RVrr", "RVri", "RVii")
    sd = recipe_state_dict({k: (Cc,) for k in leaves}, 5)
    L = SimpleNamespace(eps=1e-5, momentum=0.1, **{k: torch.from_numpy(v).to(dev) for k, v in sd.items()})
    W = [ptr(getattr(L, k)) for k in leaves[:5]]
    R = [ptr(getattr(L, k)) for k in leaves[5:]]
    alpha = torch.tensor([0.25], device=dev)
    # ComplexBatchNorm buffers
    cnb = int(lib.clskd_cbn_stats_blocks(rows, Cn))
    cpart = torch.empty(cnb * Cc * 5, dtype=torch.float64, device=dev)
    coef, stats = torch.empty(6, Cc, device=dev), torch.empty(8, Cc, device=dev)
    cbb = int(lib.clskd_cbn_bwd_blocks(rows, Cn))
    cwork = torch.empty(int(lib.clskd_cbn_bwd_workspace(cbb, Cn)), dtype=torch.float64, device=dev)
    cg = [torch.empty(Cc, device=dev) for _ in range(5)]
    cda = torch.empty(1, device=dev)
    # BatchNorm buffers
    gamma, beta = torch.ones(Cn, device=dev), torch.zeros(Cn, device=dev)
    rm, rv = torch.zeros(Cn, device=dev), torch.ones(Cn, device=dev)
    bnb = int(lib.clskd_bn_partial_blocks(rows, Cn))
    bpart = torch.empty(bnb * Cn * 2, dtype=torch.float64, device=dev)
    bcoef, mv = torch.empty(2 * Cn, device=dev), torch.empty(2, Cn, device=dev)
    sc, sh = bcoef.data_ptr(), bcoef.data_ptr() + 4 * Cn
    bbb = int(lib.clskd_bn_bwd_blocks(rows, Cn))
    bwork = torch.empty(int(lib.clskd_bn_bwd_workspace(bbb, Cn)), dtype=torch.float64, device=dev)
    bg, bb, bda = torch.empty(Cn, device=dev), torch.empty(Cn, device=dev), torch.empty(1, device=dev)
    F32 = ops._dt(x)

    def c_stats():
        chk(lib.clskd_cbn_stats_partial(ptr(x), rows, Cn, ptr(cpart), cnb, st()), "cbn_stats")

    def c_fin():
        chk(lib.clskd_cbn_finalize(ptr(cpart), cnb, rows, Cn, *W, 1e-5, *R, 0.1, 1, ptr(coef),
                                   ptr(stats), st()), "cbn_finalize")

    def b_stats():
        chk(lib.clskd_bn_stats_partial(ptr(x), rows, Cn, ptr(bpart), bnb, F32, st()), "bn_stats")

    def b_fin():
        chk(lib.clskd_bn_finalize(ptr(bpart), bnb, rows, Cn, ptr(gamma), ptr(beta), 1e-5, ptr(rm),
                                  ptr(rv), 0.1, 1, sc, sh, ptr(mv[0]), ptr(mv[1]), st()), "bn_finalize")

    pairs = {
        "stats_partial": (c_stats, b_stats, n4),
        "stats_partial + finalize": (lambda: (c_stats(), c_fin()), lambda: (b_stats(), b_fin()), n4),
        "apply + PReLU (out of place)": (
            lambda: chk(lib.clskd_cbn_apply(ptr(x), ptr(y), rows, Cn, ptr(coef), ptr(alpha), st()),
                        "cbn_apply"),
            lambda: chk(lib.clskd_bn_apply(ptr(x), ptr(y), rows, Cn, sc, sh, ptr(alpha), F32, st()),
                        "bn_apply"), 2 * n4),
        "bwd (reduce + finalize + apply)": (
            lambda: chk(lib.clskd_cbn_bwd(ptr(x), ptr(dy), rows, Cn, ptr(coef), ptr(stats), *W[:3],
                                          ptr(alpha), ptr(cwork), cbb, *[ptr(t) for t in cg],
                                          ptr(cda), ptr(dx), 0, 0, st()), "cbn_bwd"),
            lambda: chk(lib.clskd_bn_bwd(ptr(x), ptr(dy), rows, Cn, sc, sh, ptr(mv[0]), ptr(mv[1]),
                                         1e-5, ptr(gamma), ptr(alpha), ptr(bwork), bbb, ptr(bg),
                                         ptr(bb), ptr(bda), ptr(dx), 0, 0, F32, st()), "bn_bwd"),
            5 * n4),
    }
    c_stats(), c_fin(), b_stats(), b_fin()  # coefficients for the apply / backward entries
    recs = []
    for kname, (fc, fb, nbytes) in pairs.items():
        mc, mb = time_pair(fc, fb, reps, runs)
        medc, medb = statistics.median(mc), statistics.median(mb)
        recs.append(dict(bench="cbn_kernel", tensor=name, shape=list(shape), kernel=kname, reps=reps,
                         runs=runs, bytes=nbytes, cbn_ms=_stat(mc), bn_ms=_stat(mb),
                         cbn_gbps=round(nbytes / medc / 1e6, 1), bn_gbps=round(nbytes / medb / 1e6, 1),
                         ratio=round(medc / medb, 3),
                         bn_spread=round((max(mb) - min(mb)) / medb, 3),
                         cbn_spread=round((max(mc) - min(mc)) / medc, 3),
                         blocks=dict(cbn_stats=cnb, bn_stats=bnb, cbn_bwd=cbb, bn_bwd=bbb),
                         gpu=torch.cuda.get_device_name(0)))
    return recs


def build(use_cbn, mode, dev):
    from clskd.model import DCCRN
    from clskd.supervised import SupervisedTraining
    from clskd.train import FlatAdam, FlatParams
    from clskd.weights import STUDENT_SEED, apply_recipe
    m = apply_recipe(DCCRN(masking_mode="E", use_clstm=True, use_cbn=use_cbn, **cfg.STUDENT),
                     STUDENT_SEED).to(dev).train()
    mod = SupervisedTraining(m, mode)
    flat = FlatParams(mod.student)
    return mod, flat, FlatAdam(flat, lr=cfg.learning_rate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=cfg.batch)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kreps", type=int, default=20)
    ap.add_argument("--mode", default="SI-SNR")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cbn.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cbn_bench: no HIP device (a CPU run gives no time)")
    dev = torch.device("cuda", 0)
    L = int(a.seconds * cfg.fs)
    T = cfg.n_frames(L)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    C0 = cfg.kernel_num_student[0]
    for name, shape in (("encoder.0", (a.batch, 128, T, C0)), ("decoder.4", (a.batch, 128, T + 1, C0))):
        for rec in kernel_records(name, shape, a.kreps, a.runs, dev):
            emit(rec)

    import sup_loss_ref as S
    from sup_train_bench import measure
    x, y = S.seeded_batch(a.batch, L, seed=1)
    batch = (x.to(dev), y.to(dev))
    mods = {u: build(u, a.mode, dev) for u in (True, False)}
    runs = {True: [], False: []}
    for _ in range(a.runs):
        for u in (True, False):  # alternated
            runs[u].append(measure(*mods[u], batch, a.steps, a.warmup))
    med = {}
    for u in (True, False):
        devms, host, wall = ([r[i] for r in runs[u]] for i in range(3))
        med[u] = statistics.median(devms)
        emit(dict(bench="cbn_train_step", use_cbn=u, loss_mode=a.mode, B=a.batch, L=L, steps=a.steps,
                  warmup=a.warmup, runs=a.runs, device_ms=_stat(devms), host_enqueue_ms=_stat(host),
                  wall_ms=_stat(wall), last_loss=runs[u][-1][3],
                  spread=round((max(devms) - min(devms)) / med[u], 3),
                  gpu=torch.cuda.get_device_name(0)))
    emit(dict(bench="cbn_train_step_ratio", loss_mode=a.mode, B=a.batch, L=L,
              cbn_over_bn_device=round(med[True] / med[False], 3)))


if __name__ == "__main__":
    main()
