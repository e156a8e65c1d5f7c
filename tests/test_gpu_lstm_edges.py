"""GPU: the LSTM recurrence kernels of csrc/lstm.hip at their time edges and in the model's
layouts, elementwise against the float64 reference of tests/lstm_ref.py.

Sequence lengths (lstm_ref.FWD_T / PRE_T / BWD_T) sit on the code's own boundaries: the multi-wave
forward's flush every CH = 32 steps and its 64-row history ring, the forward kernels' two-step
unroll with a clamped prefetch, the single-wave backward's ring of four operand sets.  Layouts: the
model's (clskd/clstm.py: the weight sets interleaved inside a row) with every stride padded past
the dense size, and once per variant the planar dense layout.  Every output buffer starts as NaN
and every padding element must keep its bits; every addressed element must be written.

Tolerance: kernel_refs.tolerance with factor 8, e32 from the plain and two 1-ulp-perturbed float32
restatements of the reference (lstm_ref.case) — nothing in it looks at a kernel's output.  One test
covers one kernel variant, loops over the sequence lengths and reports every failing length with
the (set, sequence, step, unit) of its worst element.  Each (variant, T) prints one LSTMEDGE line
(profiles/lstm_edges.txt).

Which kernel ran: the LSTM entries record no kernel name; the route is asserted through what the
library offers — the knob read back and, for H = 32, clskd_lstm_pre_capable, which is true exactly
when the single-wave kernel takes lstm_recurrent."""
import contextlib
import ctypes

import pytest
import torch

import lstm_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -777.0   # padding of the in-place / read-only input buffers
NWS, NSEQ = L.NWS, L.NSEQ


# ------------------------------------------------------------------------------------------
# strided buffers with guarded padding
# ------------------------------------------------------------------------------------------
class Buf:
    """A flat fp32 buffer addressed as `shape` at the element `strides` (last axis dense), 16
    guard elements behind the last addressed one.  fill: the value of every element that `data`
    (a tensor of `shape`, or None) does not set."""

    def __init__(self, shape, strides, fill, data=None):
        self.shape, self.strides = tuple(shape), tuple(strides) + (1,)
        n = 1 + sum((d - 1) * s for d, s in zip(self.shape, self.strides)) + 16
        host = torch.full((n,), fill, dtype=torch.float32)
        if data is not None:
            host.as_strided(self.shape, self.strides).copy_(data)
        self.before = host.clone()
        self.mask = torch.zeros(n, dtype=torch.bool)
        self.mask.as_strided(self.shape, self.strides).fill_(True)
        self.dev = host.to(DEV)

    def read(self, what, written=True):
        """The addressed view after a launch.  Everything outside it must hold its earlier bits;
        written: every addressed element must be finite (an output), else the whole buffer must be
        unchanged (an input)."""
        after = self.dev.cpu()
        same = after.view(torch.int32) == self.before.view(torch.int32)
        keep = ~self.mask if written else torch.ones_like(self.mask)
        bad = (~same & keep).nonzero().flatten()
        assert bad.numel() == 0, f"{what}: {bad.numel()} elements outside the addressed set changed, first at {int(bad[0])}"
        view = after.as_strided(self.shape, self.strides)
        if written:
            nf = (~torch.isfinite(view)).nonzero()
            assert nf.numel() == 0, f"{what}: {nf.shape[0]} addressed elements not written, first {nf[0].tolist()}"
        return view.clone()


def model_gx(H, T, nws, nseq):
    """clstm.py's interleaved layout with padded rows: (ws, seq, t) strides of gx / pre / dgates."""
    gx_t = nws * 4 * H + 8
    return (4 * H, T * gx_t + 16, gx_t)


def model_out(H, T, nws, nseq):
    """Padded [nws][nseq][T][H]: (ws, seq, t) strides of out / dh."""
    o_t = H + 4
    o_seq = T * o_t + 8
    return (nseq * o_seq + 12, o_seq, o_t)


def planar(W, T, nws, nseq):
    return (nseq * T * W, T * W, W)


def strides_of(layout, H, T, nws, nseq):
    if layout == "model":
        return model_gx(H, T, nws, nseq), model_out(H, T, nws, nseq)
    return planar(4 * H, T, nws, nseq), planar(H, T, nws, nseq)


def guarded(n):
    """A dense NaN buffer of exactly n elements inside a larger NaN one (the entries take the
    cell-state buffer without strides): (view, whole)."""
    whole = torch.full((n + 32,), NAN, device=DEV)
    return whole[16:16 + n], whole


def guards_intact(whole, n):
    w = whole.cpu()
    return bool(torch.isnan(w[:16]).all() and torch.isnan(w[16 + n:]).all())


# ------------------------------------------------------------------------------------------
# knobs, comparison, report
# ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def knobs(**kv):
    """Set dispatch knobs (CLSKD_<NAME>=value), read each back, restore on exit.  A value the
    product library does not offer (an experiments-only knob off its default) skips the test."""
    from clskd import _lib
    prev = {}
    try:
        for k, v in kv.items():
            name = "CLSKD_" + k
            try:
                prev[name] = _lib.set_knob(name, v)
            except RuntimeError as e:
                if "CLSKD_EXPERIMENTS" in str(e):
                    pytest.skip(f"{name}={v} is not settable in the product library: {e}")
                raise
            got = ctypes.c_int32(-1)
            assert _lib.load().clskd_get_knob(name.encode(), ctypes.byref(got)) == 0 and got.value == v
        yield
    finally:
        for name, v in prev.items():
            _lib.set_knob(name, v)


class Report:
    """Collects one line per (variant, T) and every miss; asserts at the end."""

    def __init__(self, variant):
        self.variant, self.lines, self.bad = variant, [], []

    def row(self, layout, T):
        self.cur = f"LSTMEDGE {self.variant} {layout} T={T}"
        self.lines.append(self.cur)
        return self

    def cmp(self, key, got, ref64, e32_tol, note=""):
        e32, tol = e32_tol
        err = (got.double() - ref64).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        worst = float(err.max())
        at = tuple(int(i) for i in torch.unravel_index(err.argmax(), err.shape))
        self.lines[-1] += f" | {key}{note} e32 {e32:.2e} tol {tol:.2e} err {worst:.2e}"
        if not worst <= tol:
            nbad = int((err > tol).sum())
            self.lines[-1] += f" MISS at (set, seq, step, unit) = {at}, {nbad} elements over"
            self.bad.append(self.lines[-1])

    def check(self, ok, text):
        if not ok:
            self.lines[-1] += f" | MISS {text}"
            self.bad.append(self.lines[-1])

    def finish(self):
        print("\n" + "\n".join(self.lines))
        assert not self.bad, "\n" + "\n".join(self.bad)


def dev(t):
    return t.contiguous().to(DEV)


# ------------------------------------------------------------------------------------------
# lstm_recurrent
# ------------------------------------------------------------------------------------------
def run_fwd(H, T, nws, nseq, layout, what):
    from clskd import ops
    cs = L.case(H, T, nws, nseq)
    gs, os_ = strides_of(layout, H, T, nws, nseq)
    gx = Buf((nws, nseq, T, 4 * H), gs, SENTINEL, cs["gx"])
    out = Buf((nws, nseq, T, H), os_, NAN)
    ops.lstm_recurrent(gx.dev, *gs, dev(cs["whh"]), nws, nseq, T, H, out.dev, *os_)
    torch.cuda.synchronize()
    gx.read(f"{what} gx", written=False)
    return cs, out.read(f"{what} out")


FWD_VARIANTS = [
    ("h32_wave", 32, dict(LSTM_NKS32=1)), ("h32_nks2", 32, dict(LSTM_NKS32=2)),
    ("h32_nks4", 32, dict(LSTM_NKS32=4)), ("h32_nks8", 32, dict(LSTM_NKS32=8)),
    ("h16", 16, {}), ("h64", 64, {}),
    ("h128_nks4", 128, dict(LSTM_NKS=4)), ("h128_nks2", 128, dict(LSTM_NKS=2)),
    ("h128_nks8", 128, dict(LSTM_NKS=8)),
]


@pytest.mark.parametrize("name,H,kn", FWD_VARIANTS, ids=[v[0] for v in FWD_VARIANTS])
def test_lstm_recurrent_time_edges(name, H, kn):
    """h of clskd_lstm_recurrent against float64, elementwise under the rule: every T of
    lstm_ref.FWD_T in the model layout, the planar layout at T = 65, CLSKD_LSTM_PRIO = 1 at
    T = 65 (0 everywhere else)."""
    from clskd import ops
    rep = Report("fwd " + name)
    with knobs(LSTM_PRIO=0, **kn):
        if H == 32:  # the route: single-wave kernel <=> the taped forward is offered
            assert ops.lstm_pre_capable(32) == (kn["LSTM_NKS32"] == 1)
        for layout, T in [("model", T) for T in L.FWD_T] + [("planar", L.PLANAR_T)]:
            cs, h = run_fwd(H, T, NWS, NSEQ, layout, f"{name} {layout} T={T}")
            rep.row(layout, T).cmp("h", h, cs["ref"]["h"], cs["tol"]["h"])
        with knobs(LSTM_PRIO=1):
            cs, h = run_fwd(H, L.PRIO_T, NWS, NSEQ, "model", f"{name} prio T={L.PRIO_T}")
            rep.row("model,prio=1", L.PRIO_T).cmp("h", h, cs["ref"]["h"], cs["tol"]["h"])
    rep.finish()


@pytest.mark.parametrize("H,T", L.SINGLE)
def test_lstm_recurrent_one_set_one_sequence(H, T):
    """nws = nseq = 1: a grid of one workgroup, no set or sequence stride applied."""
    rep = Report(f"fwd h{H}_1x1")
    with knobs(LSTM_PRIO=0):
        cs, h = run_fwd(H, T, 1, 1, "model", f"h{H} 1x1 T={T}")
        rep.row("model", T).cmp("h", h, cs["ref"]["h"], cs["tol"]["h"])
    rep.finish()


# ------------------------------------------------------------------------------------------
# lstm_recurrent_pre
# ------------------------------------------------------------------------------------------
def run_pre(T, with_cells, what):
    """The taped forward in place over gx (model layout, two sets): (case, h, pre, cells)."""
    from clskd import ops
    H = 32
    cs = L.case(H, T, NWS, NSEQ)
    gs, os_ = strides_of("model", H, T, NWS, NSEQ)
    gx = Buf((NWS, NSEQ, T, 4 * H), gs, SENTINEL, cs["gx"])
    out = Buf((NWS, NSEQ, T, H), os_, NAN)
    n = NWS * NSEQ * T * H
    cells, whole = guarded(n) if with_cells else (None, None)
    ops.lstm_recurrent_pre(gx.dev, *gs, dev(cs["whh"]), NWS, NSEQ, T, H, out.dev, *os_, cbuf=cells)
    torch.cuda.synchronize()
    c = None
    if with_cells:
        assert guards_intact(whole, n), f"{what}: cell-state buffer written outside its {n} slots"
        c = cells.cpu().view(NWS, NSEQ, T, H)
        assert torch.isfinite(c).all(), f"{what}: cell-state slots not written"
    # the padding inside gx keeps its sentinel; every addressed element now holds a pre-activation
    return cs, out.read(f"{what} out"), gx.read(f"{what} gx in place"), c, cells


@pytest.mark.parametrize("with_cells", [False, True], ids=["nocbuf", "cbuf"])
def test_lstm_recurrent_pre_time_edges(with_cells):
    """clskd_lstm_recurrent_pre in place over gx in the model layout: h bitwise lstm_recurrent's,
    pre-activations and cell states against float64 under the rule, sentinel padding kept."""
    from clskd import ops
    rep = Report("pre h32_" + ("cbuf" if with_cells else "nocbuf"))
    with knobs(LSTM_PRIO=0, LSTM_NKS32=1, LSTM_PRE=1):
        assert ops.lstm_pre_capable(32)
        for T in L.PRE_T:
            what = f"pre T={T}"
            cs, h, pre, c, _ = run_pre(T, with_cells, what)
            _, h_plain = run_fwd(32, T, NWS, NSEQ, "model", what + " plain")
            rep.row("model", T)
            rep.check(torch.equal(h, h_plain), "h differs from lstm_recurrent's bits")
            rep.cmp("h", h, cs["ref"]["h"], cs["tol"]["h"])
            rep.cmp("pre", pre, cs["ref"]["pre"], cs["tol"]["pre"])
            if with_cells:
                rep.cmp("c", c, cs["ref"]["c"], cs["tol"]["c"])
    rep.finish()


# ------------------------------------------------------------------------------------------
# lstm_bwd
# ------------------------------------------------------------------------------------------
def run_bwd(H, T, layout, what, cells=None):
    """Gate gradients from the float64 pre-activations rounded to float32 and a random dh."""
    from clskd import ops
    cs = L.case(H, T, NWS, NSEQ)
    gs, ds = strides_of(layout, H, T, NWS, NSEQ)
    pre = Buf((NWS, NSEQ, T, 4 * H), gs, SENTINEL, cs["ref"]["pre"].float())
    dh = Buf((NWS, NSEQ, T, H), ds, SENTINEL, cs["dh"])
    dg = Buf((NWS, NSEQ, T, 4 * H), gs, NAN)
    ops.lstm_bwd(pre.dev, gs, dh.dev, ds, dev(cs["whh"]), NWS, NSEQ, T, H, dg.dev, gs, cells=cells)
    torch.cuda.synchronize()
    pre.read(f"{what} pre", written=False)
    dh.read(f"{what} dh", written=False)
    return cs, dg.read(f"{what} dgates")


BWD_VARIANTS = [(f"h{H}_{tag}", H, kn) for H in (16, 32) for tag, kn in (
    ("wave_pin", dict(LSTM_BWD_WAVE=1, LSTM_BWD_PIN=1)), ("wave_nopin", dict(LSTM_BWD_WAVE=1, LSTM_BWD_PIN=0)),
    ("multi", dict(LSTM_BWD_WAVE=0, LSTM_BWD_PIN=1)))] + [("h64", 64, {}), ("h128", 128, {})]


@pytest.mark.parametrize("name,H,kn", BWD_VARIANTS, ids=[v[0] for v in BWD_VARIANTS])
def test_lstm_bwd_time_edges(name, H, kn):
    """dgates of clskd_lstm_bwd against float64 autograd, elementwise under the rule: every T of
    lstm_ref.BWD_T (all residues mod 4, T < 4) in the model layout with padded dh, the planar
    layout at T = 65; for the single-wave H = 32 kernel also with the taped forward's cell states
    (c_ready = 1), which must agree with the scanning run within 1e-5 / 1e-6."""
    from clskd import ops
    rep = Report("bwd " + name)
    with_cells = H == 32 and kn["LSTM_BWD_WAVE"] == 1
    with knobs(LSTM_PRIO=0, LSTM_NKS32=1, LSTM_PRE=1, **kn):
        for layout, T in [("model", T) for T in L.BWD_T] + [("planar", L.PLANAR_T)]:
            what = f"{name} {layout} T={T}"
            cs, dg = run_bwd(H, T, layout, what)
            rep.row(layout, T).cmp("dgates", dg, cs["ref"]["dgx"], cs["tol"]["dgx"])
            if with_cells and layout == "model":
                assert ops.lstm_pre_capable(32)
                _, _, _, _, cells = run_pre(T, True, what + " taped forward")
                before = cells.clone()
                _, dg_c = run_bwd(H, T, layout, what + " cells", cells=cells)
                rep.check(torch.equal(before, cells), "c_ready = 1 run wrote the cell states")
                rep.cmp("dgates", dg_c, cs["ref"]["dgx"], cs["tol"]["dgx"], note="(cells)")
                gap = (dg_c.double() - dg.double()).abs() - (1e-6 + 1e-5 * dg.double().abs())
                rep.lines[-1] += f" | cells-vs-scan over 1e-5/1e-6 by {float(gap.max()):.2e}"
                rep.check(float(gap.max()) <= 0.0, "cells= and scan disagree beyond 1e-5 / 1e-6")
    rep.finish()


# ------------------------------------------------------------------------------------------
# lstm_cell
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", L.HIDDEN)
def test_lstm_cell_carried_70_steps(H):
    """clskd_lstm_cell carried for 70 steps with clstm.py's gx strides (4H, 8H), padded state and
    output strides: out bitwise h at every step, h against step t of the float64 recurrence under
    the rule, state padding untouched.  (No bit equality with the offline kernels: the
    activations are shared, the k-sum order is not.)"""
    from clskd import ops
    T = L.CELL_STEPS
    cs = L.case(H, T, NWS, NSEQ)
    s_seq = H + 4
    ss = (NSEQ * s_seq + 8, s_seq)
    o_seq = H + 8
    os_ = (NSEQ * o_seq + 4, o_seq)
    zero = torch.zeros(NWS, NSEQ, H)
    h = Buf((NWS, NSEQ, H), ss, SENTINEL, zero)
    c = Buf((NWS, NSEQ, H), ss, SENTINEL, zero)
    gx = dev(cs["gx"].permute(2, 1, 0, 3))   # [T][nseq][nws * 4H]
    whh = dev(cs["whh"])
    outs, hs = [], []
    for t in range(T):
        out = Buf((NWS, NSEQ, H), os_, NAN)
        ops.lstm_cell(gx[t], 4 * H, NWS * 4 * H, whh, NWS, NSEQ, H, h.dev, c.dev, *ss, out.dev, *os_)
        outs.append(out)
        hs.append(h.dev.clone())
    torch.cuda.synchronize()
    rep = Report(f"cell h{H}")
    got = torch.empty(NWS, NSEQ, T, H)
    rep.row("model", T)
    for t in range(T):
        o = outs[t].read(f"cell h{H} out step {t}")
        ht = hs[t].cpu().as_strided(h.shape, h.strides)
        rep.check(torch.equal(o, ht), f"out != h at step {t}")
        got[:, :, t] = o
    h.read(f"cell h{H} h state")
    cfin = c.read(f"cell h{H} c state")
    rep.cmp("h", got, cs["ref"]["h"], cs["tol"]["h"])
    rep.cmp("c(T-1)", cfin[:, :, None], cs["ref"]["c"][:, :, -1:], cs["tol"]["c"])
    rep.finish()


# ------------------------------------------------------------------------------------------
# refusals: no kernel is launched
# ------------------------------------------------------------------------------------------
def test_lstm_entries_refuse_bad_shapes():
    """T = 0, nseq = 0, an unbuilt hidden size and a misaligned whh come back as the library's
    error through ops (an exception naming the entry), the outputs untouched.  (tests/test_abi.py
    asserts the null-pointer refusal of clskd_lstm_recurrent only.)"""
    from clskd import ops
    H, T = 32, 4
    gx = torch.zeros(NWS, NSEQ, T, 4 * H, device=DEV)
    pre = gx.clone()
    out = torch.full((NWS, NSEQ, T, H), NAN, device=DEV)
    dg = torch.full((NWS, NSEQ, T, 4 * H), NAN, device=DEV)
    wbuf = torch.zeros(NWS * 4 * 48 * 48 + 4, device=DEV)
    whh = wbuf[:NWS * 4 * H * H]
    off4 = wbuf[1:1 + NWS * 4 * H * H]
    assert whh.data_ptr() % 16 == 0 and off4.data_ptr() % 16 == 4
    gs, os_ = planar(4 * H, T, NWS, NSEQ), planar(H, T, NWS, NSEQ)
    for fn, entry in ((ops.lstm_recurrent, "lstm"), (ops.lstm_recurrent_pre, "lstm_pre")):
        with pytest.raises(RuntimeError, match=rf"clskd {entry} failed \(-1\): {entry}: empty shape"):
            fn(gx, *gs, whh, NWS, NSEQ, 0, H, out, *os_)
        with pytest.raises(RuntimeError, match=rf"clskd {entry} failed \(-1\): {entry}: empty shape"):
            fn(gx, *gs, whh, NWS, 0, T, H, out, *os_)
        with pytest.raises(RuntimeError, match=rf"clskd {entry} failed \(-4\): {entry}: whh must be 16-byte aligned"):
            fn(gx, *gs, off4, NWS, NSEQ, T, H, out, *os_)
    g48, o48 = planar(4 * 48, T, NWS, NSEQ), planar(48, T, NWS, NSEQ)
    with pytest.raises(RuntimeError, match=r"clskd lstm failed \(-1\): lstm: hidden size 48 not built"):
        ops.lstm_recurrent(gx, *g48, wbuf, NWS, 1, 1, 48, out, *o48)
    with pytest.raises(RuntimeError, match=r"clskd lstm_pre failed \(-1\): lstm_pre: H=48"):
        ops.lstm_recurrent_pre(gx, *g48, wbuf, NWS, 1, 1, 48, out, *o48)
    with pytest.raises(RuntimeError, match=r"clskd lstm_bwd failed \(-1\): lstm_bwd: hidden size 48 not built"):
        ops.lstm_bwd(pre, g48, out, o48, wbuf, NWS, 1, 1, 48, dg, g48)
    # ops.lstm_bwd sizes the cell-state buffer itself (an empty one has no address), so the empty
    # shapes of lstm_bwd go to the library directly, with a buffer that is never touched
    from clskd import _lib
    for nseq, Tn in ((0, T), (NSEQ, 0)):
        rc = _lib.load().clskd_lstm_bwd(pre.data_ptr(), *gs, out.data_ptr(), *os_, whh.data_ptr(), NWS, nseq,
                                        Tn, H, out.data_ptr(), 0, dg.data_ptr(), *gs, None)
        assert rc == -1 and b"lstm_bwd: empty shape" in _lib.load().clskd_last_error()
    st = torch.zeros(NWS, NSEQ, 48, device=DEV)
    with pytest.raises(RuntimeError, match=r"clskd lstm_cell failed \(-1\): lstm_cell: hidden size 48 not built"):
        ops.lstm_cell(gx, 4 * 48, 8 * 48, wbuf, NWS, 1, 48, st, st.clone(), 48, 48, out, 48, 48)
    with pytest.raises(RuntimeError, match=r"clskd lstm_cell failed \(-1\): lstm_cell: empty shape"):
        ops.lstm_cell(gx, 4 * H, 8 * H, whh, NWS, 0, H, st, st.clone(), NSEQ * H, H, out, NSEQ * H, H)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(dg).all() and bool((pre == 0).all())
