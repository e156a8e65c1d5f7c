"""Backward pass of the asteroid ``DCCRNet_mini`` (clskd.asteroid) on libclskd_hip.so: the
reverse of ``DCCRNet_mini.run(x, True, tape=...)``, in the style of ``backward.dccrn_backward``.

Every data gradient of a GEMM (complex convs, polyphase transposed convs, the complex Linear,
the LSTM projections, the STFTFB synthesis) is another launch of the implicit-GEMM conv engine
with a transposed packed weight; every weight gradient is ``ops.conv_wgrad`` over the forward's
own descriptor; the bounded mask and the OnReIm BatchNorm + PReLU have the kernels of
csrc/mini_bwd.hip; packed-operand gradients map back onto the ``re_module`` / ``im_module``
parameters through ``backward.unpack_maps``, so each parameter receives both of its products.
Everything runs fp32 on the exact engines; every reduction has a fixed order, so two backward
passes over one tape give the same bits.  The filterbanks are buffers and are not trained.
"""
import torch

from . import backward as bw
from . import clstm, ops
from .asteroid import DCCRNet_mini
from .backward import _cbias_fn, _dec_dgrad_w, _empty, _enc_pack_fn, _scatter, _tw, unpack_maps
from .ops import OutMap, Seg, SegGeom, seg_bftc


def _cat2_fn(a, b):
    return torch.cat([a.reshape(-1), b.reshape(-1)]).reshape(-1, 1)


def _dec_pack_fn(taps_kf, nprev):
    """DCCRNet_mini._dec_w's packing of one parity: [Co, (tap, [prev re, im | skip re, im])]."""
    def fn(wr, wi):
        top = torch.cat([wr, wi], 1)
        bot = torch.cat([-wi, wr], 1)
        w = torch.cat([top, bot], 0)
        ci = wr.shape[0]
        ns = ci - nprev
        w = torch.cat([w[0:nprev], w[ci:ci + nprev], w[nprev:ci], w[ci + nprev:ci + nprev + ns]], 0)
        taps = [(kf, kt) for kf in taps_kf for kt in (0, 1)]
        w = torch.stack([w[:, :, kf, kt] for kf, kt in taps], 0).permute(2, 0, 1)
        return w.reshape(w.shape[0], -1)
    return fn


def _bn_prelu_bwd(entry, dy, pg, acc):
    """OnReIm(BatchNorm2d) + OnReIm(PReLU) backward of one taped block: returns d raw."""
    raw, coef, mv, norm, act, gamma, alpha = entry
    Co = raw.shape[-1]
    dev = raw.device
    draw = _empty(raw.shape, dev)
    dgam, dbet, dalp = _empty((Co,), dev), _empty((Co,), dev), _empty((2,), dev)
    ops.bn_bwd_reim(raw, dy, coef[:Co], coef[Co:], mv[0], mv[1], norm.re_module.eps, gamma, alpha,
                    draw, dgam, dbet, dalp)
    half = unpack_maps(("cat2", Co // 2), _cat2_fn, [(Co // 2,), (Co // 2,)], 1, dev)
    _scatter(dgam, half, [pg.get(norm.re_module.weight), pg.get(norm.im_module.weight)], acc)
    _scatter(dbet, half, [pg.get(norm.re_module.bias), pg.get(norm.im_module.bias)], acc)
    _scatter(dalp, unpack_maps(("cat2", 1), _cat2_fn, [(1,), (1,)], 1, dev),
             [pg.get(act.re_module.weight), pg.get(act.im_module.weight)], acc)
    return draw


def mini_backward(model, tape, d_wav, pg, acc_params=False):
    """Gradients of a loss with dL/d wav = d_wav [B][L] (fp32, read only) w.r.t. the parameters
    of `model` (a DCCRNet_mini), over the tape of model.run(x, True, tape=tape).
    pg: dict parameter -> fp32 gradient tensor (contiguous, the parameter's shape); parameters
    missing from it are skipped.  acc_params: add into pg instead of overwriting."""
    m = model
    B, T, L = tape["B"], tape["T"], tape["L"]
    spec, enc, mask = tape["spec"], tape["enc"], tape["mask"]
    dev = spec.device
    if d_wav.shape != (B, L) or d_wav.dtype != torch.float32 or not d_wav.is_contiguous():
        raise ValueError("mini_backward: d_wav must be a contiguous fp32 [B, L] tensor")
    batch = bw._BATCH_SCATTERS and not acc_params and bw._SCATTERS is None
    if batch:
        bw._SCATTERS = []
    try:
        _mini_backward(m, tape, d_wav, pg, acc_params, B, T, L, spec, enc, mask, dev)
        if batch and bw._SCATTERS:
            ops.index_gather_jobs(bw._SCATTERS)
    finally:
        if batch:
            bw._SCATTERS = None


def _mini_backward(m, tape, d_wav, pg, acc, B, T, L, spec, enc, mask, dev):
    TAPS = DCCRNet_mini._DEC_TAPS
    # ---------------- pad_x_to_y + plain overlap-add + STFTFB synthesis, reverse: the analysis-
    # shaped framing GEMM of d_wav against the transposed synthesis filters (samples at or past
    # 100 (T + 3) are padding zeros of the forward and are never read)
    _, ws = m._fb_w()  # [400][516]
    wt = _tw(("mini_syn_t", id(m)), ws,
             lambda: ops.pack_weight(ws[:, :516].t().contiguous().unsqueeze(1), 400))
    dest = _empty((B, T, 516), dev)
    ops.conv([Seg(d_wav, 0, SegGeom(100, L, 0, 100, 1, L // 100))], [(0, kt) for kt in range(4)],
             B, 1, T, 516, wt, None, dest, OutMap(T * 516, 0, 516), mfma_only=True)
    # ---------------- BoundComplexMask('tanh') * spectrum, reverse
    dmask = _empty(mask.shape, dev)
    ops.mask_bdt_bwd(spec, mask, T, dest, dmask)

    # ---------------- output layer and decoders 5..1 (the first takes cat([rnn_out, enc[5]]):
    # the Identity decoder's cat), reverse
    nenc = len(enc)
    rnn_out = tape["rnn_out"]
    dec = tape["dec"]
    dec_mods = list(m.masker.decoders)[1:] + [m.masker.output_layer[0]]
    g_enc = [_empty(t.shape, dev) for t in enc]
    g_dec = [_empty(t.shape, dev) for t in dec]
    g_rnn = _empty(rnn_out.shape, dev)
    for d in range(len(dec_mods) - 1, -1, -1):
        mod = dec_mods[d]
        is_out = d == len(dec_mods) - 1
        deconv = mod if is_out else mod.deconv
        rm, im_ = deconv.re_module, deconv.im_module
        prev = rnn_out if d == 0 else dec[d - 1]
        skip = enc[nenc - 1 - d]
        F, Ti = prev.shape[1], prev.shape[2]
        Cp, Cs_ = prev.shape[-1], skip.shape[-1]
        Ci = Cp + Cs_
        Co = 2 * rm.out_channels
        draw = dmask if is_out else _bn_prelu_bwd(tape["dec_bn"][d], g_dec[d], pg, acc)
        segs = [seg_bftc(prev), seg_bftc(skip)]
        # weight gradients: both polyphase parities into one concatenated packed buffer
        packs = [m._dec_w(deconv, p, Cp // 2) for p in (0, 1)]
        Kps = [packs[p][0].shape[1] for p in (0, 1)]
        dwcat = _empty((Co * (Kps[0] + Kps[1]),), dev)
        dbias = _empty((Co,), dev) if rm.bias is not None else None
        omap_t = (Ti + 1) * Co
        for p in (0, 1):
            taps = [(dF, -kt) for _, dF in TAPS[p] for kt in (0, 1)]
            dw = dwcat[Co * Kps[0] * p:Co * (Kps[0] + Kps[1] * p)].view(Co, Kps[p])
            ops.conv_wgrad(segs, taps, B, F, Ti + 1, Co, draw,
                           OutMap(2 * F * omap_t, omap_t, Co, of_mul=2, of_add=p), dw, dbias,
                           accumulate=False, accumulate_bias=p == 1)
        K0, K1 = Kps

        def fn(wr, wi, K0=K0, K1=K1, nprev=Cp // 2):  # parity 0 as [Co][K0], then parity 1 as [Co][K1]
            a = _dec_pack_fn([kf for kf, _ in TAPS[0]], nprev)(wr, wi)
            b = _dec_pack_fn([kf for kf, _ in TAPS[1]], nprev)(wr, wi)
            a = torch.cat([a, a.new_zeros(a.shape[0], K0 - a.shape[1])], 1)
            b = torch.cat([b, b.new_zeros(b.shape[0], K1 - b.shape[1])], 1)
            return torch.cat([a.reshape(-1), b.reshape(-1)]).reshape(1, -1)

        shapes = [tuple(rm.weight.shape), tuple(im_.weight.shape)]
        maps = unpack_maps(("mini_dec", Co, Cp, Cs_, K0, K1), fn, shapes, Co * (K0 + K1), dev)
        _scatter(dwcat, maps, [pg.get(rm.weight), pg.get(im_.weight)], acc)
        if dbias is not None:
            bmaps = unpack_maps(("cbias", Co), _cbias_fn, [(Co // 2,), (Co // 2,)], 1, dev)
            _scatter(dbias, bmaps, [pg.get(rm.bias), pg.get(im_.bias)], acc)
        # data gradients: one stride-2 gather over the raw-output gradient per destination; each
        # destination's first contribution (the skips' other one, an encoder's or the LSTM's
        # data gradient, accumulates later)
        dseg = Seg(draw, 0, SegGeom(Co, 2 * F * omap_t, omap_t, Co, 2 * F, Ti + 1))
        taps_b = [(p - 2 * dF, kt) for p in (0, 1) for _, dF in TAPS[p] for kt in (0, 1)]
        for s0, Cs, dst in ((0, Cp, g_rnn if d == 0 else g_dec[d - 1]), (Cp, Cs_, g_enc[nenc - 1 - d])):
            wtd = _tw(("mini_dec_t", id(m), d, s0), packs[0][0],
                      lambda: _dec_dgrad_w(packs, Ci, s0, Cs))
            ops.conv([dseg], taps_b, B, F, Ti, Cs, wtd, None, dst, OutMap(F * Ti * Cs, Ti * Cs, Cs),
                     stride_f=2)

    # ---------------- complex Linear (K = 2H row product: re = [Wr | -Wi], im = [Wi | Wr]), reverse
    e6 = enc[-1]
    D4, C6 = e6.shape[1], e6.shape[-1]
    Ch = C6 // 2
    Ti = e6.shape[2]
    rnn = m.masker.encoders[-1].rnn
    lin = m.masker.encoders[-1].linear
    Lr, Li = lin.re_module, lin.im_module
    H = rnn.rnns[0].re_module.rnn.hidden_size
    N = Ch * D4
    wre, _, wim, _ = m._lin_w()
    Kl = wre.shape[1]
    r_out = tape["r_out"]
    segs = [Seg(r_out[h], 0, SegGeom(H, Ti * H, 0, H, 1, Ti)) for h in range(2)]
    omap = OutMap(D4 * Ti * C6, 0, C6, 1, Ti * C6, D4)
    dwl = _empty((2, N, Kl), dev)
    dbl = _empty((2 * N,), dev)
    for half in range(2):
        ops.conv_wgrad(segs, [(0, 0)], B, 1, Ti, N, g_rnn, omap, dwl[half], dbl[half * N:(half + 1) * N],
                       dy_offset=half * Ch)
    _scatter(dwl, unpack_maps(("mini_lin", N, H), lambda a, b: torch.cat(
        [torch.cat([a, -b], 1), torch.cat([b, a], 1)], 0), [(N, H), (N, H)], Kl, dev),
        [pg.get(Lr.weight), pg.get(Li.weight)], acc)
    _scatter(dbl, unpack_maps(("cbias", 2 * N), _cbias_fn, [(N,), (N,)], 1, dev),
             [pg.get(Lr.bias), pg.get(Li.bias)], acc)
    d_out = [_empty((B, Ti, H), dev), _empty((B, Ti, H), dev)]
    gsegs = [Seg(g_rnn, s * Ch, SegGeom(Ch, D4 * Ti * C6, Ti * C6, C6, D4, Ti)) for s in range(2)]
    for h in range(2):
        # K order (tap f, [re | im] product, channel c) over rows n = c * D4 + f of wre / wim
        wtl = _tw(("mini_lin_t", id(m), h), wre, lambda: ops.pack_weight(
            torch.stack([wre[:, h * H:(h + 1) * H], wim[:, h * H:(h + 1) * H]], 0)
            .reshape(2, Ch, D4, H).permute(3, 2, 0, 1).contiguous().reshape(H, D4, 2 * Ch),
            D4 * 2 * Ch))
        ops.conv(gsegs, [(f, 0) for f in range(D4)], B, 1, Ti, H, wtl, None, d_out[h],
                 OutMap(Ti * H, 0, H), mfma_only=True)

    # ---------------- two complex LSTM layers, reverse
    in0 = [([seg_bftc(e6, c0=half * Ch, C=Ch)], [(f, 0) for f in range(D4)]) for half in range(2)]
    clstm.backward(d_out, tape, m._lstm_w,
                   [(r.re_module.rnn, r.im_module.rnn) for r in rnn.rnns], in0, g_enc[-1], m, pg, acc)

    # ---------------- encoders 6..1 (5x2 kernel, F stride 2, no time padding: T shrinks by one
    # per block, so a data gradient reads zeros outside the block's [0, To)), reverse
    for i in range(nenc - 1, -1, -1):
        blk = m.masker.encoders[i]
        cr, ci_ = blk.conv.re_module, blk.conv.im_module
        draw = _bn_prelu_bwd(tape["enc_bn"][i], g_enc[i], pg, acc)
        src = tape["xin"] if i == 0 else enc[i - 1]
        Cin = src.shape[-1]
        _, Fo, To, Co = draw.shape
        wp = m._enc_w(i)
        dw = _empty(wp.shape, dev)
        ops.conv_wgrad([seg_bftc(src)], [(kf - 2, kt) for kf in range(5) for kt in range(2)], B, Fo,
                       To, Co, draw, OutMap(Fo * To * Co, To * Co, Co), dw, None, stride_f=2)
        maps = unpack_maps(("enc", Co, Cin), _enc_pack_fn,
                           [tuple(cr.weight.shape), tuple(ci_.weight.shape)], wp.shape[1], dev)
        _scatter(dw, maps, [pg.get(cr.weight), pg.get(ci_.weight)], acc)
        if i == 0:
            continue  # the spectrum comes from a fixed filterbank: no data gradient
        dseg = Seg(draw, 0, SegGeom(Co, Fo * To * Co, To * Co, Co, Fo, To))
        Tin = To + 1
        for p in (0, 1):
            kfs = [kf for kf in range(5) if kf % 2 == p]
            taps_b = [((p - kf + 2) // 2, -kt) for kf in kfs for kt in range(2)]
            wte = _tw(("mini_enc_t", id(m), i, p), wp, lambda: ops.pack_weight(
                wp[:, :10 * Cin].reshape(Co, 5, 2, Cin)[:, p::2].permute(3, 1, 2, 0)
                .reshape(Cin, len(kfs) * 2, Co).contiguous(), len(kfs) * 2 * Co))
            ops.conv([dseg], taps_b, B, Fo, Tin, Cin, wte, None, g_enc[i - 1],
                     OutMap(2 * Fo * Tin * Cin, Tin * Cin, Cin, of_mul=2, of_add=p), accumulate=True)
