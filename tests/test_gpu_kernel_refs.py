"""The small kernels of the training backward and the losses, each against the float64 references
of tests/kernel_refs.py: the ReviewKD fusion backward with its folds and BatchNorm partials, the
nearest down-sum, the framing pad / overlap-add / log-magnitude / complex-combine backwards with
their forwards, SI-SNR, the SPKD gradient pair spkd_grad + gram_bwd, and the BatchNorm forward
kernels (statistics, finalize, eval coefficients, apply + PReLU) at channel counts that are no
power of two.

One tolerance rule for every floating-point comparison (kernel_refs.tolerance): with ref64 the
float64 reference on exactly the kernel's inputs (bf16 inputs rounded first, float arguments as
the float32 the kernel receives) and ref32 the same torch expression evaluated in float32 on the
CPU, e32 = max|ref32 - ref64| and every element must satisfy

    |got - ref64| <= 8 * e32 + 4 * 2^-24 * max|ref64|.

The factor 8 covers another summation order (16-lane xor trees, fixed-order slab sums), device
expf / logf / atan2f against the host libm at a couple of ulp, and FMA contraction; the second term
keeps the bound non-zero where the float32 evaluation happens to be exact.  The bound never uses
the kernel's output.  Kernels that only copy, permute, negate or zero-fill are compared bitwise.
Elements whose float64 decision value lies within a stated margin of a gate (the clamp of the
overlap-add, the sign and the power floor of the log-magnitude loss) are left out, and their
share is asserted to stay under 1 %.  Every case prints one line `case e32 err tol` (err and tol
at the element with the largest err / tol); profiles/kernel_refs_margins.txt keeps a run's lines.
"""
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
bf = torch.bfloat16
f32 = torch.float32
f64 = torch.float64


def _dev(t):
    return None if t is None else t.to(DEV)


def _f32(v):
    """A Python float as the float32 a kernel argument carries."""
    return float(torch.tensor(v, dtype=f32))


def _check(case, got, ref64, ref32, keep=None, factor=8.0, scale=None):
    e32, tol = R.tolerance(ref64, ref32, keep, factor, scale)
    err = (got.detach().double().cpu() - ref64).abs()
    tol_t = torch.broadcast_to(torch.as_tensor(tol, dtype=f64), err.shape)
    if keep is not None:
        err, tol_t = err[keep], tol_t[keep]
    err, tol_t = err.reshape(-1), tol_t.reshape(-1)
    i = int(torch.argmax(err / tol_t))
    print(f"KREF {case} e32={e32:.3e} err={err[i].item():.3e} tol={tol_t[i].item():.3e}")
    assert torch.isfinite(err).all(), case
    assert (err <= tol_t).all(), (case, e32, err[i].item(), tol_t[i].item())


# ------------------------------------------------------------------------------------------
# A. ReviewKD fusion
# ------------------------------------------------------------------------------------------
def _abf_kernel(d, adt, gdt, coef, mv1):
    """abf_fuse_bwd on the case's inputs with activations stored `adt` and gradient maps `gdt`;
    returns dx, dyup and the block-summed BatchNorm partials [64][3] (fp64) or None."""
    from clskd import ops
    x1, res = _dev(d["x1"].to(adt)), _dev(d["res"].to(adt))
    dout = _dev(d["dout"].to(gdt))
    dnext = None if d["dnext"] is None else _dev(d["dnext"].to(gdt))
    dx = torch.full(x1.shape, 9.0, device=DEV, dtype=gdt)
    dyup = torch.full(x1.shape, 9.0, device=DEV, dtype=gdt)
    part, nblk = ops.abf_fuse_bwd(x1, res, _dev(d["w"]), _dev(d["b"]), _dev(coef), dout, dx, dyup,
                                  dnext=dnext, mv1=_dev(mv1))
    torch.cuda.synchronize()
    if part is not None:
        part = part.view(nblk, 64, 3).sum(0).cpu()
    return dx, dyup, part


def _abf_refs(d, adt, gdt, coef, mv1):
    out = []
    for dt in (f64, f32):
        x1, res, dout, dnext = [None if t is None else t.to(s).to(dt) for t, s in
                                ((d["x1"], adt), (d["res"], adt), (d["dout"], gdt), (d["dnext"], gdt))]
        w, b, cf, mv = R.cast(dt, d["w"], d["b"], coef, mv1)
        out.append((R.abf_fuse_bwd(x1, res, w, b, cf, dout, dnext, mv), (x1, res, w, b, cf)))
    return out


def _abf_compare(tag, d, adt, coef, mv1):
    (r64, in64), (r32, in32) = _abf_refs(d, adt, f32, coef, mv1)
    dx, dyup, part = _abf_kernel(d, adt, f32, coef, mv1)
    _check(f"{tag}/dx", dx, r64[0], r32[0])
    _check(f"{tag}/dyup", dyup, r64[1], r32[1])
    if mv1 is not None:
        # fp64 sums of fp32 terms: the rule with max|ref64| replaced by the sum of the terms'
        # magnitudes, per channel
        for k, name in enumerate(("sum_dx", "sum_dx_xhat")):
            _check(f"{tag}/{name}", part[:, k], r64[2][k], r32[2][k], scale=r64[3][k])
        assert (part[:, 2] == 0).all()
    return in64, in32


@pytest.mark.parametrize("name,adt", [("model", f32), ("mix", f32), ("general", f32), ("bare", f32),
                                      ("double", f32), ("model", bf), ("general", bf)])
def test_abf_fuse_bwd_against_fp64(name, adt):
    """dx, dyup and the conv1-BatchNorm partials of abf_fuse_bwd on every fold path of the next
    level's gradient: rf=2 / rt=1 (the model), the 1x / 2x mix, 2x on both axes (the only grid
    that reads all four children of the fast path), the general search loops on both axes, and
    no next level at all (nor partials, nor folded affine).  On fp32 activations the
    forward abf_fuse runs on the same inputs against the same reference, which pins the forward's
    nearest_src and the backward's nearest_src_b to one map."""
    from clskd import ops
    case = R.ABF_CASES[name]
    d = R.abf_inputs(case)
    coef, mv1 = (None, None) if name == "bare" else (d["coef"], d["mv1"])
    tag = f"abf_bwd[{name},{'bf16' if adt == bf else 'fp32'}]"
    in64, in32 = _abf_compare(tag, d, adt, coef, mv1)
    if adt == f32:
        out = torch.empty(d["x1"].shape, device=DEV)
        ops.abf_fuse(_dev(d["x1"]), _dev(d["res"]), _dev(d["w"]), _dev(d["b"]), out, x_coef=_dev(coef))
        torch.cuda.synchronize()
        _check(f"abf_fwd[{name}]", out, R.abf_fuse(*in64), R.abf_fuse(*in32))


def test_abf_fuse_bwd_paired_iteration_and_tail():
    """A grid in the model's form (F doubles, T equal) with nslots < B*F*T < 2*nslots, nslots =
    16 * clskd_abf_fuse_bwd_blocks read from the library: every pixel slot runs one paired
    iteration or one single-pixel tail (`two == false`), and pixels sit beyond the first
    grid-stride."""
    from clskd import ops
    blocks = lambda B, Fn, T: int(ops.lib().clskd_abf_fuse_bwd_blocks(B, Fn, T))
    B, Fn = 2, 128
    cap_slots = 16 * blocks(64, 1024, 1024)  # the capped grid's pixel slots
    T = (cap_slots * 11 // 8) // (B * Fn) | 1
    case = (B, Fn, T, Fn // 2, T, 2 * Fn, T)
    nslots = 16 * blocks(B, Fn, T)
    assert nslots < B * Fn * T < 2 * nslots, (nslots, case)
    d = R.abf_inputs(case, seed=7)
    _abf_compare(f"abf_bwd[large {B}x{Fn}x{T}]", d, f32, d["coef"], d["mv1"])


@pytest.mark.parametrize("name", ["model", "general"])
def test_abf_fuse_bwd_bf16_maps_are_the_fp32_path_rounded_once(name):
    """bf16 gradient maps (dout / dnext / dx / dyup): the arithmetic stays fp32, so on
    bf16-representable gradients the outputs are the fp32-storage path's rounded once, bitwise."""
    d = R.abf_inputs(R.ABF_CASES[name], seed=3)
    for k in ("dout", "dnext"):
        d[k] = d[k].to(bf).float()
    fx, fy, _ = _abf_kernel(d, bf, f32, d["coef"], d["mv1"])
    hx, hy, _ = _abf_kernel(d, bf, bf, d["coef"], d["mv1"])
    assert torch.equal(hx, fx.to(bf))
    assert torch.equal(hy, fy.to(bf))


@pytest.mark.parametrize("Fn,T,Fr,Tr", R.DOWN_CASES)
@pytest.mark.parametrize("gdt", [f32, bf])
def test_nearest_down_sum_against_fp64(Fn, T, Fr, Tr, gdt):
    from clskd import ops
    gen = torch.Generator().manual_seed(Fn * 100 + T)
    for C in (4, 64):
        g = torch.randn(2, Fn, T, C, generator=gen).to(gdt)
        prior = torch.randn(2, Fr, Tr, C, generator=gen)
        for acc in (False, True):
            out = _dev(prior.clone())
            ops.nearest_down_sum(_dev(g), out, accumulate=acc)
            torch.cuda.synchronize()
            p = prior if acc else None
            r64 = R.nearest_down_sum(g.double(), (Fr, Tr), None if p is None else p.double())
            r32 = R.nearest_down_sum(g.float(), (Fr, Tr), p)
            _check(f"down_sum[{Fn}x{T}->{Fr}x{Tr},C{C},{'bf16' if gdt == bf else 'fp32'},acc{int(acc)}]",
                   out, r64, r32)


# ------------------------------------------------------------------------------------------
# B. waveform tail
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.PAD_CASES))
def test_frame_pad_and_backward(name):
    """frame_pad bitwise (a copy), frame_pad_bwd (a sum of at most three terms) by the rule: into
    a contiguous dx, and accumulated into a row-strided view whose other columns keep a sentinel."""
    from clskd import ops
    L, pad, Lp, mode = R.PAD_CASES[name]
    B = 3
    gen = torch.Generator().manual_seed(L + pad)
    xbuf = torch.randn(B, L + 3, generator=gen)
    xp = torch.full((B, Lp), 9.0, device=DEV)
    ops.frame_pad(_dev(xbuf)[:, :L], pad, Lp, mode, xp)
    torch.cuda.synchronize()
    assert torch.equal(xp.cpu(), R.frame_pad(xbuf[:, :L], pad, Lp, mode))
    dxp = torch.randn(B, Lp, generator=gen)
    dx = torch.full((B, L), 9.0, device=DEV)
    ops.frame_pad_bwd(_dev(dxp), L, pad, mode, dx)
    torch.cuda.synchronize()
    _check(f"frame_pad_bwd[{name}]", dx, R.frame_pad_bwd(dxp.double(), L, pad, mode),
           R.frame_pad_bwd(dxp, L, pad, mode))
    prior = torch.randn(B, L + 7, generator=gen)
    buf = _dev(prior.clone())
    ops.frame_pad_bwd(_dev(dxp), L, pad, mode, buf[:, :L], accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(buf[:, L:].cpu(), prior[:, L:])
    _check(f"frame_pad_bwd[{name},strided,acc]", buf[:, :L],
           R.frame_pad_bwd(dxp.double(), L, pad, mode, prior[:, :L].double()),
           R.frame_pad_bwd(dxp, L, pad, mode, prior[:, :L]))


def test_frame_pad_reflect_needs_pad_below_length():
    """Reflect padding with pad >= L is refused by the argument check, before any launch."""
    from clskd import ops
    x = torch.zeros(1, 4, device=DEV)
    xp = torch.zeros(1, 12, device=DEV)
    with pytest.raises(RuntimeError, match="reflect pad"):
        ops.frame_pad(x, 4, 12, 1, xp)
    with pytest.raises(RuntimeError, match="reflect pad"):
        ops.frame_pad_bwd(xp, 4, 4, 1, x)
    with pytest.raises(RuntimeError, match="reflect pad"):
        ops.frame_pad_bwd(xp, 4, 5, 1, x)


@pytest.mark.parametrize("name", sorted(R.OLA_CASES))
@pytest.mark.parametrize("clamp", [0, 1])
def test_ola_and_backward(name, clamp):
    """ola_hop and ola_bwd.  The clamp is continuous, so the forward compares every sample; its
    gradient jumps at |pre| = 1, so frame entries whose float64 pre-clamp sample lies within
    1e-4 of the gate are left out (under 1 % of them).  Entries of samples outside
    [trim, trim + out_len) get exactly 0."""
    from clskd import ops
    case = R.OLA_CASES[name]
    B, T, win, hop, trim, out_len = case
    frames, window, dwav = R.ola_inputs(case)
    wav = torch.full((B, out_len), 9.0, device=DEV)
    ops.ola_hop(_dev(frames), _dev(window), hop, out_len, trim, clamp, wav)
    dfr = torch.full((B, T, win), 9.0, device=DEV)
    ops.ola_bwd(_dev(frames), _dev(window), _dev(dwav), hop, out_len, trim, clamp, dfr)
    torch.cuda.synchronize()
    w64, _ = R.ola(frames.double(), window.double(), hop, out_len, trim, clamp)
    w32, _ = R.ola(frames, window, hop, out_len, trim, clamp)
    _check(f"ola[{name},clamp{clamp}]", wav, w64, w32)
    d64, pre = R.ola_bwd(frames.double(), window.double(), dwav.double(), hop, out_len, trim, clamp)
    d32, _ = R.ola_bwd(frames, window, dwav, hop, out_len, trim, clamp)
    near = (pre.abs() - 1.0).abs() < R.OLA_GATE_MARGIN if clamp else torch.zeros_like(pre, dtype=torch.bool)
    near_f, inside = R.frames_of_samples(near, T, win, hop, trim, False)
    inside = inside.expand(B, T, win)
    assert near_f[inside].double().mean().item() <= 0.01
    _check(f"ola_bwd[{name},clamp{clamp}]", dfr, d64, d32, keep=~near_f)
    assert (dfr.cpu()[~inside] == 0).all()
    assert (d64[~inside] == 0).all()


@pytest.mark.parametrize("name", sorted(R.STFT_CASES))
def test_stft_mag_loss_and_backward(name):
    """stft_mag_loss ([sc, mag], written and accumulated) and stft_mag_loss_bwd: row pitches with
    and without pad columns (the gradient's pad columns exactly 0), bins under the 1e-7 power
    floor and bins where Y equals X (gradient exactly 0 for both)."""
    from clskd import ops
    case = R.STFT_CASES[name]
    nb, rows, ld, ldd = case
    X, Y = R.stft_inputs(case)
    fsc, fmag, scale = _f32(0.1), _f32(0.2), _f32(0.37)
    prior = torch.tensor([0.3, 0.7])
    Xd, Yd = _dev(X), _dev(Y)
    out = ops.stft_mag_loss(Xd, Yd, nb, fsc, fmag)
    acc = ops.stft_mag_loss(Xd, Yd, nb, fsc, fmag, out2=_dev(prior.clone()), accumulate=True)
    dX = torch.full((rows, ldd), 9.0, device=DEV)
    ops.stft_mag_loss_bwd(Xd, Yd, nb, scale, dX)
    torch.cuda.synchronize()
    _check(f"stft_mag_loss[{name}]", out, R.stft_mag_loss(X.double(), Y.double(), nb, fsc, fmag),
           R.stft_mag_loss(X, Y, nb, fsc, fmag))
    _check(f"stft_mag_loss[{name},acc]", acc,
           R.stft_mag_loss(X.double(), Y.double(), nb, fsc, fmag, prior.double()),
           R.stft_mag_loss(X, Y, nb, fsc, fmag, prior))
    left = R.stft_left_out(X.double(), Y.double(), nb)
    assert left.double().mean().item() <= 0.01
    keep = torch.cat([~left, ~left, torch.ones(rows, ldd - 2 * nb, dtype=torch.bool)], 1)
    _check(f"stft_mag_loss_bwd[{name}]", dX, R.stft_mag_loss_bwd(X.double(), Y.double(), nb, scale, ldd),
           R.stft_mag_loss_bwd(X, Y, nb, scale, ldd), keep=keep)
    got = dX.cpu()
    assert (got[:, 2 * nb:] == 0).all()
    for half in (0, nb):
        assert (got[:, half:half + nb:7] == 0).all()  # under the floor
        assert (got[:, half:half + nb:5] == 0).all()  # Y equals X
    assert (got[:, 1] != 0).all()  # an ordinary bin


@pytest.mark.parametrize("L", R.SISNR_LENGTHS)
def test_sisnr_rows_against_fp64(L):
    from clskd import ops
    s1, s2 = R.sisnr_inputs(L)
    eps = _f32(1e-8)
    got = ops.sisnr_rows(_dev(s1)[:, :L], _dev(s2)[:, :L], eps)
    torch.cuda.synchronize()
    r64 = R.sisnr_rows(s1.double()[:, :L], s2.double()[:, :L], eps)
    if L >= 255:
        assert (r64.abs() < 20).all(), r64
    _check(f"sisnr_rows[L{L}]", got, r64, R.sisnr_rows(s1[:, :L], s2[:, :L], eps))


def test_complex_combine_and_backward_bitwise():
    from clskd import ops
    gen = torch.Generator().manual_seed(11)
    B, n = 3, 37
    rr, ii, ir, ri, dre, dim = [torch.randn(B, n, generator=gen) for _ in range(6)]
    ref_r, ref_i = R.complex_combine(rr, ii, ir, ri)
    for dt in (f32, bf):
        ro = torch.empty(B, n, device=DEV, dtype=dt)
        io = torch.empty(B, n, device=DEV, dtype=dt)
        ops.complex_combine(_dev(rr), _dev(ii), _dev(ir), _dev(ri), ro, io)
        torch.cuda.synchronize()
        assert torch.equal(ro.cpu(), ref_r.to(dt)) and torch.equal(io.cpu(), ref_i.to(dt))
    dh = torch.full((2, 2 * B, n), 9.0, device=DEV)
    ops.complex_combine_bwd(_dev(dre), _dev(dim), dh)
    torch.cuda.synchronize()
    assert torch.equal(dh.cpu(), R.complex_combine_bwd(dre, dim))


@pytest.mark.parametrize("B,T,ld,re0,im0,Fn", R.SPEC_CASES)
def test_spec_bftc_bitwise(B, T, ld, re0, im0, Fn):
    from clskd import ops
    spec = torch.randn(B, T, ld, generator=torch.Generator().manual_seed(T))
    out = torch.full((B, Fn, T, 2), 9.0, device=DEV)
    ops.spec_bftc(_dev(spec), re0, im0, Fn, out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), R.spec_bftc(spec, re0, im0, Fn))


# ------------------------------------------------------------------------------------------
# C. SPKD gradient
# ------------------------------------------------------------------------------------------
P, CTOT, CS, C0 = 37, 24, 8, 8
CHUNK = 128  # elements per row per slab: 16 positions of 8 channels -> slabs of 16, 16, 5


@pytest.mark.parametrize("B", R.SPKD_BATCHES)
@pytest.mark.parametrize("batchmean", [True, False])
@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_spkd_grad_then_gram_bwd_against_fp64(B, batchmean, scale):
    """M = dG + dG^T from the Gram slabs (spkd_grad: B*B entries over 1024 threads — every thread
    at B = 32, idle threads in the last phase at B = 29, 40 phases at B = 5) and dz = M z
    (gram_bwd) against float64 autograd of the SPKD term w.r.t. the student's z.  Grams as the
    backward builds them: GramSlabs over an fp32 channel slice and a bf16 teacher view, three
    slabs each with a ragged last one."""
    from clskd import ops
    zs, zt = R.spkd_inputs(B)
    scale = _f32(scale)
    zs_d, zt_d = _dev(zs), _dev(zt)
    vs = ops.GramView(zs_d, 0, P * CTOT, P, CTOT, C0, CS)
    vt = ops.GramView(zt_d, 0, P * CS, P, CS, 0, CS)
    slabs = ops.GramSlabs([vs, vt], B, chunk_elems=CHUNK)
    assert all(n >= 3 for _, n in slabs.refs) and P % (CHUNK // CS) != 0
    M = ops.spkd_grad([slabs.refs[0]], [slabs.refs[1]], B, batchmean, scale, device=DEV)
    dz = torch.full((B, P, CTOT), 9.0, device=DEV)
    ops.gram_bwd([(vs, M[0], dz, P * CTOT, CTOT, C0, False)], B)
    torch.cuda.synchronize()
    zsv = zs[:, :, C0:C0 + CS].reshape(B, -1)
    M64, dz64, Gs, Gt = R.spkd_grad(zsv.double(), zt.double().reshape(B, -1), batchmean, scale)
    M32, dz32, _, _ = R.spkd_grad(zsv, zt.float().reshape(B, -1), batchmean, scale)
    # every Gram entry well away from 0: the sign(G) term of the gradient is smooth
    assert Gs.abs().min() >= 1e-3 * Gs.abs().max() and Gt.abs().min() >= 1e-3 * Gt.abs().max()
    got = dz.cpu()
    other = torch.ones(CTOT, dtype=torch.bool)
    other[C0:C0 + CS] = False
    assert (got[:, :, other] == 9.0).all()
    tag = f"B{B},{'batchmean' if batchmean else 'sum'},scale{scale:.2f}"
    if B == 1:
        assert (M64 == 0).all() and (M.cpu() == 0).all() and (got[:, :, C0:C0 + CS] == 0).all()
        return
    _check(f"spkd_grad[{tag}]", M[0], M64, M32)
    _check(f"gram_bwd[{tag}]", got[:, :, C0:C0 + CS].reshape(B, -1), dz64, dz32)


@pytest.mark.parametrize("B", [5, 32])
def test_gram_bwd_views_accumulate_and_offsets(B):
    """gram_bwd alone on a given M, two jobs in one launch: an fp32 channel slice written at
    o_c0 = 4 inside wider rows (the other channels keep a sentinel), and a bf16 view with a
    folded affine, z = bf16(fma(raw, sc, sh)); written and accumulated."""
    from clskd import ops
    gen = torch.Generator().manual_seed(40 + B)
    zs, _ = R.spkd_inputs(B, seed=1)
    M = torch.randn(B, B, generator=gen) * 0.01
    raw = torch.randn(B, P, 16, generator=gen).to(bf)
    aff = torch.cat([torch.rand(16, generator=gen) + 0.5, torch.randn(16, generator=gen) * 0.1])
    za = (raw[:, :, 8:16].double() * aff[8:16].double() + aff[24:32].double()).float().to(bf)
    z0 = zs[:, :, C0:C0 + CS]
    v0 = ops.GramView(_dev(zs), 0, P * CTOT, P, CTOT, C0, CS)
    v1 = ops.GramView(_dev(raw), 0, P * 16, P, 16, 8, 8, _dev(aff))
    Md = _dev(M)
    for acc in (False, True):
        p0 = torch.randn(B, P, 16, generator=gen)
        p1 = torch.randn(B, P, 8, generator=gen)
        o0, o1 = _dev(p0.clone()), _dev(p1.clone())
        ops.gram_bwd([(v0, Md, o0, P * 16, 16, 4, acc), (v1, Md, o1, P * 8, 8, 0, acc)], B)
        torch.cuda.synchronize()
        o0 = o0.cpu()
        assert torch.equal(o0[:, :, :4], p0[:, :, :4]) and torch.equal(o0[:, :, 12:], p0[:, :, 12:])
        for tag, got, z, prior in (("fp32_slice", o0[:, :, 4:12], z0, p0[:, :, 4:12]),
                                   ("bf16_affine", o1, za, p1)):
            refs = []
            for dt in (f64, f32):
                r = torch.einsum("bk,kpc->bpc", M.to(dt), z.to(dt))
                refs.append(r + prior.to(dt) if acc else r)
            _check(f"gram_bwd[{tag},B{B},acc{int(acc)}]", got, refs[0], refs[1])


# ------------------------------------------------------------------------------------------
# F. BatchNorm + PReLU at channel counts that are no power of two (csrc/norm.hip)
# ------------------------------------------------------------------------------------------
# The statistics kernel maps lanes to (row lane, channel quad): with C/4 not dividing 256 the last
# lanes idle; the apply kernel keeps one group of 8 channels per lane only while C/8 divides its
# grid stride.  16-bit storage: the reference is the float64 result on the rounded inputs, rounded
# once to the storage type, and one ulp of that type is allowed on top of the rule.
f16 = torch.float16
EPS, MOM = 1e-5, 0.1


def _ulp(ref, dtype):
    """One unit in the last place of dtype at each |ref| (0 for float32: the rule alone)."""
    if dtype == f32:
        return torch.zeros_like(ref, dtype=f64)
    _, e = torch.frexp(ref.to(dtype).double().abs().clamp(min=float(torch.finfo(dtype).tiny)))
    return torch.ldexp(torch.full_like(ref, torch.finfo(dtype).eps, dtype=f64), e - 1)


def _check_stored(case, got, ref64, ref32, dtype):
    """got (stored as dtype) against ref64 rounded once to dtype: the rule plus one ulp."""
    e32, tol = R.tolerance(ref64, ref32)
    want = ref64.to(dtype).double()
    err = (got.detach().double().cpu() - want).abs()
    tol_t = tol + _ulp(want, dtype)
    i = int(torch.argmax(err / tol_t))
    print(f"KREF {case} e32={e32:.3e} err={err.reshape(-1)[i].item():.3e} "
          f"tol={tol_t.reshape(-1)[i].item():.3e}")
    assert torch.isfinite(err).all(), case
    assert (err <= tol_t).all(), (case, e32, err.reshape(-1)[i].item(), tol_t.reshape(-1)[i].item())


def _bn_case(rows, C, dt):
    """Inputs as the kernel receives them (x rounded to its storage type) in float64 / float32."""
    d = R.bn_inputs(rows, C)
    d["x"] = d["x"].to(dt).float()
    return d, {k: v.double() for k, v in d.items()}


@pytest.mark.parametrize("dt", [f32, bf], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", R.BN_ROWS)
@pytest.mark.parametrize("C", R.BN_CHANNELS)
def test_batch_norm_train_against_fp64(C, rows, dt):
    """ops.batch_norm_bftc(train=True): statistics, finalize, apply + PReLU, stats_out and one
    running update.  rows = 1: the unbiased factor rows / (rows - 1) is undefined (torch refuses
    the input); the kernel then updates running_var with the biased variance, 0 — finite — and
    only the batch mean, the biased variance and y are compared beside that statement."""
    from clskd import ops
    d32, d64 = _bn_case(rows, C, dt)
    alpha = torch.tensor([0.25])
    args = lambda d: (d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], EPS, MOM,  # noqa: E731
                      alpha.to(d["x"].dtype))
    r64, r32 = R.batch_norm_train(*args(d64)), R.batch_norm_train(*args(d32))
    x = _dev(d32["x"].to(dt)).view(1, rows, 1, C)
    y = torch.full_like(x, float("nan"))
    rm, rv = _dev(d32["rm"].clone()), _dev(d32["rv"].clone())
    mv = torch.full((2, C), float("nan"), device=DEV)
    _, coef = ops.batch_norm_bftc(x, y, _dev(d32["gamma"]), _dev(d32["beta"]), rm, rv, True, MOM,
                                  EPS, 1, alpha=_dev(alpha), stats_out=(mv[0], mv[1]),
                                  return_coef=True)
    torch.cuda.synchronize()
    tag = f"bn_train C={C} rows={rows} {str(dt)[6:]}"
    _check(f"{tag} mean", mv[0], r64["mean"], r32["mean"])
    _check(f"{tag} var", mv[1], r64["var"], r32["var"])
    if rows == 1:  # running_var <- (1 - momentum) running_var + momentum * 0: finite
        assert torch.equal(mv[1].cpu(), torch.zeros(C)) and torch.isfinite(rv).all()
    else:
        _check(f"{tag} scale", coef[:C], r64["scale"], r32["scale"])
        _check(f"{tag} shift", coef[C:], r64["shift"], r32["shift"])
    _check(f"{tag} running_var", rv, r64["rv"], r32["rv"])
    _check(f"{tag} running_mean", rm, r64["rm"], r32["rm"])
    _check_stored(f"{tag} y", y.view(rows, C), r64["y"], r32["y"], dt)


@pytest.mark.parametrize("dt", [f32, bf], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", R.BN_ROWS)
@pytest.mark.parametrize("C", R.BN_CHANNELS)
def test_batch_norm_eval_against_fp64(C, rows, dt):
    """ops.batch_norm_bftc(train=False): clskd_bn_eval_coeffs + apply + PReLU; the running
    statistics stay as they are."""
    from clskd import ops
    d32, d64 = _bn_case(rows, C, dt)
    alpha = torch.tensor([0.25])
    args = lambda d: (d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], EPS,  # noqa: E731
                      alpha.to(d["x"].dtype))
    r64, r32 = R.batch_norm_eval(*args(d64)), R.batch_norm_eval(*args(d32))
    x = _dev(d32["x"].to(dt)).view(1, rows, 1, C)
    y = torch.full_like(x, float("nan"))
    rm, rv = _dev(d32["rm"].clone()), _dev(d32["rv"].clone())
    _, coef = ops.batch_norm_bftc(x, y, _dev(d32["gamma"]), _dev(d32["beta"]), rm, rv, False, MOM,
                                  EPS, 1, alpha=_dev(alpha), return_coef=True)
    torch.cuda.synchronize()
    tag = f"bn_eval C={C} rows={rows} {str(dt)[6:]}"
    assert torch.equal(rm.cpu(), d32["rm"]) and torch.equal(rv.cpu(), d32["rv"])
    _check(f"{tag} scale", coef[:C], r64["scale"], r32["scale"])
    _check(f"{tag} shift", coef[C:], r64["shift"], r32["shift"])
    _check_stored(f"{tag} y", y.view(rows, C), r64["y"], r32["y"], dt)


def _apply_case(rows, C, dt, slopes, inplace):
    """ops.bn_apply (no slope / one slope) or clskd_bn_apply_reim (two) on given coefficients."""
    from clskd import ops
    d32, d64 = _bn_case(rows, C, dt)
    al = [None if a is None else torch.tensor(a) for a in (list(slopes) + [None, None])[:2]]
    ref = lambda d: R.bn_affine(d["x"], d["scale"], d["shift"],  # noqa: E731
                                *[None if a is None else a.to(d["x"].dtype) for a in al])
    r64, r32 = ref(d64), ref(d32)
    x = _dev(d32["x"].to(dt)).view(1, rows, 1, C)
    y = x if inplace else torch.full_like(x, float("nan"))
    coef = _dev(torch.cat([d32["scale"], d32["shift"]]).contiguous())
    if len(slopes) == 2:
        alpha = _dev(torch.tensor(list(slopes)))
        sc = coef.data_ptr()
        ops.check(ops.lib().clskd_bn_apply_reim(x.data_ptr(), y.data_ptr(), rows, C, sc, sc + 4 * C,
                                                alpha.data_ptr(), ops._dt(x), ops._stream()),
                  "bn_apply_reim")
    else:
        out = ops.bn_apply(x, y, coef, _dev(torch.tensor([slopes[0]])) if slopes else None)
        assert out is y
    torch.cuda.synchronize()
    _check_stored(f"bn_apply C={C} rows={rows} {str(dt)[6:]} slopes={slopes}"
                  + (" in place" if inplace else ""), y.view(rows, C), r64, r32, dt)


@pytest.mark.parametrize("dt", [f32, bf, f16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("slopes", [(), (0.25,), (0.25, 0.05)], ids=["affine", "prelu", "reim"])
@pytest.mark.parametrize("rows", R.BN_ROWS)
@pytest.mark.parametrize("C", R.BN_CHANNELS)
def test_bn_apply_against_fp64(C, rows, slopes, dt):
    _apply_case(rows, C, dt, slopes, inplace=False)


@pytest.mark.parametrize("slopes", [(0.25,), (0.25, 0.05)], ids=["prelu", "reim"])
@pytest.mark.parametrize("C", R.BN_CHANNELS)
def test_bn_apply_in_place(C, slopes):
    _apply_case(4864, C, f32, slopes, inplace=True)


@pytest.mark.parametrize("slopes", [(0.25,), (0.25, 0.05)], ids=["prelu", "reim"])
def test_bn_apply_lanes_that_change_channel_group(slopes):
    """More items than the largest grid (4096 x 256) at C/8 = 3: the lanes that visit a second
    item find it in another channel group and reload their coefficients."""
    rows, C = R.BN_APPLY_LARGE
    assert rows * C // 8 > 4096 * 256 and (4096 * 256) % (C // 8) != 0
    _apply_case(rows, C, f32, slopes, inplace=False)
