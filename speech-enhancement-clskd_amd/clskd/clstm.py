"""The complex-LSTM stack of DCCRN and DCCRNet_mini (tools_for_model.py:138-174): the layer loop
of the forward (taped or not), of one streaming hop, and of the backward, once for both models.

Per layer: one input-projection GEMM per input half (real, imag) into ``gx`` [2][B][T][8H]
(gate rows of the real LSTM | the imag LSTM), one recurrence over the 2 weight sets x 2B
sequences into ``hs`` [2][2B][T][H], and the complex combine real = rr - ii, imag = ri + ir.
What differs between the models stays with them: where layer 0 reads its input (``in0``: per
half the (segs, taps) of its GEMM), how the weights are packed (``weights``), the storage type
of the layer outputs, and the projection after the stack.

The same loops run the real-LSTM bottleneck of DCCRN(use_clstm=False) (DCCRN.py:101-108,
192-197): ``in0`` then has one entry, and everything above holds with one weight set — ``gx``
[1][B][T][4H], one recurrence over 1 set x B sequences into ``hs`` [1][B][T][H], no combine (the
layer output is ``hs`` itself).  With S = len(in0) weight sets a layer is S input GEMMs of 4HS
gate rows and one recurrence over S sets x SB sequences.
"""
import types

import torch

from . import ops
from .ops import OutMap, Seg, SegGeom


def _project(li, in0, r_in, weights, B, T, H, gx):
    """The input-projection GEMMs of layer li (one per input half) into gx; returns (wp, bias,
    whh)."""
    S = len(in0)
    for half in range(S):
        if li == 0:
            segs, taps = in0[half]
        else:
            segs, taps = [Seg(r_in[half], 0, SegGeom(H, T * H, 0, H, 1, T))], [(0, 0)]
        wp, bias, whh = weights(li, segs)
        ops.conv(segs, taps, B, 1, T, S * 4 * H, wp, bias, gx[half],
                 OutMap(T * S * 4 * H, 0, S * 4 * H))
    return wp, bias, whh


def layer_view(lstm, k):
    """Layer k of a multi-layer nn.LSTM under the parameter names of a one-layer one (what
    backward() scatters into)."""
    return types.SimpleNamespace(**{f"{n}_l0": getattr(lstm, f"{n}_l{k}")
                                    for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")})


def forward(in0, weights, n_layers, B, T, H, out_kw, store_cells=True, tape=None):
    """The stack over [B][T] frames.  weights(li, segs) -> (wp, bias, whh) of layer li for a GEMM
    reading `segs`; out_kw: device / dtype of the layer outputs (ro, io).  With a tape,
    tape["lstm"] receives one dict(gx, hs, r_in, pre, cells) per layer; where the recurrence can
    (ops.lstm_pre_capable) it leaves the gate pre-activations in gx (pre = True) and, with
    store_cells, the cell states in cells.  Returns the per-layer [(ro, io)] — for one weight set
    (len(in0) == 1, fp32 outputs) the per-layer [(hs [B][T][H],)]."""
    f32 = dict(device=out_kw["device"], dtype=torch.float32)
    S = len(in0)
    G = S * 4 * H
    r_in = None
    lstm_io = []
    for li in range(n_layers):
        gx = torch.empty(S, B, T, G, **f32)
        whh = _project(li, in0, r_in, weights, B, T, H, gx)[2]
        hs = torch.empty(S, S * B, T, H, **f32)
        # taped: the recurrence leaves the gate pre-activations in gx (the backward's `pre`)
        pre = tape is not None and ops.lstm_pre_capable(H)
        cells = None
        if pre:  # ... and its cell states (the backward then skips its cell-state scan)
            cells = torch.empty(S * S * B * T * H, **f32) if store_cells else None
            ops.lstm_recurrent_pre(gx, 4 * H, T * G, G, whh, S, S * B, T, H, hs,
                                   S * B * T * H, T * H, H, cbuf=cells)
        else:
            ops.lstm_recurrent(gx, 4 * H, T * G, G, whh, S, S * B, T, H, hs,
                               S * B * T * H, T * H, H)
        if tape is not None:
            tape.setdefault("lstm", []).append(dict(gx=gx, hs=hs, r_in=r_in, pre=pre,
                                                    cells=cells))
        if S == 1:
            assert out_kw["dtype"] == torch.float32
            r_in = (hs.view(B, T, H),)
            lstm_io.append(r_in)
            continue
        ro = torch.empty(B, T, H, **out_kw)
        io = torch.empty(B, T, H, **out_kw)
        ops.complex_combine(hs[0, :B], hs[1, B:], hs[0, B:], hs[1, :B], ro, io)
        r_in = (ro, io)
        lstm_io.append(r_in)
    return lstm_io


def hop(in0, weights, n_layers, B, H, gx, h, c, hs, rio):
    """One frame of the stack with carried state (the per-layer streaming classes): h[li] / c[li]
    are updated in place, gx [2][B][8H] and hs [2][2B][H] are scratch, rio[li] = (ro, io)
    receive the layer outputs.  Returns the last layer's (ro, io)."""
    r_in = None
    for li in range(n_layers):
        whh = _project(li, in0, r_in, weights, B, 1, H, gx)[2]
        ops.lstm_cell(gx, 4 * H, 8 * H, whh, 2, 2 * B, H, h[li], c[li], 2 * B * H, H, hs,
                      2 * B * H, H)
        ro, io = rio[li]
        ops.complex_combine(hs[0, :B], hs[1, B:], hs[0, B:], hs[1, :B], ro, io)
        r_in = (ro, io)
    return r_in


def backward(d_out, tape, weights, lstms, in0, g_in0, owner, pg, acc):
    """Reverse of forward(tape=...).  d_out: the gradients [B][T][H] of the last layer's (ro, io);
    weights(li) -> the fp32 (wp, bias, whh); lstms[li] = the (real, imag) nn.LSTM pair whose
    parameters receive the gradients (through pg, see backward._scatter) — one nn.LSTM (or
    layer_view) per weight set, so a 1-tuple for the real-LSTM stack, whose d_out is the 1-list of
    the gradient of the last layer's hs; in0 as in forward;
    g_in0 [B][D4][T][C6]: the gradient of layer 0's BFTC input, accumulated into; owner: the
    model (its id keys the transposed-weight cache).
    A layer whose tape holds only gx gets the pre-activations rebuilt in place in gx, once per
    tape (lt["pre"] is set: a second backward over the tape finds them there)."""
    from . import backward as bw  # backward imports this module
    B, T, H = d_out[0].shape
    dev = d_out[0].device
    _, D4, _, C6 = g_in0.shape
    S = len(in0)
    G = S * 4 * H
    Ch = C6 // S  # input channels per half
    _empty, _scatter, _tw, unpack_maps = bw._empty, bw._scatter, bw._tw, bw.unpack_maps
    for li in range(len(lstms) - 1, -1, -1):
        lt = tape["lstm"][li]
        gx, hs = lt["gx"], lt["hs"]
        sets = lstms[li]
        R = sets[0]
        wp, _, whh = weights(li)
        if S == 2:
            dh = _empty((2, 2 * B, T, H), dev)
            ops.complex_combine_bwd(d_out[0], d_out[1], dh)
        else:
            dh = d_out[0].view(1, B, T, H)
        whp = _tw(("whh_p", id(owner), li), whh,
                  lambda: torch.stack([ops.pack_weight(whh[ws].unsqueeze(1), H) for ws in range(S)]))
        if not lt["pre"]:
            # gate pre-activations gx + h_{t-1} W_hh^T over the saved history, in place in gx
            for ws in range(S):
                hseg = Seg(hs, ws * S * B * T * H, SegGeom(H, T * H, 0, H, 1, T))
                ops.conv([hseg], [(0, -1)], S * B, 1, T, 4 * H, whp[ws], None, gx,
                         OutMap(T * G, 0, G), out_offset=ws * 4 * H, accumulate=True)
            lt["pre"] = True
        dg = _empty((S, B, T, G), dev)
        st = (4 * H, T * G, G)
        ops.lstm_bwd(gx, st, dh, (S * B * T * H, T * H, H), whh, S, S * B, T, H, dg, st,
                     cells=lt.get("cells"))
        # W_hh gradient per weight set: rows (seq, t) x the shifted history h_{t-1}
        Kh = whp.shape[2]
        dwhh = _empty((S, 4 * H, Kh), dev)
        for ws in range(S):
            hseg = Seg(hs, ws * S * B * T * H, SegGeom(H, T * H, 0, H, 1, T))
            ops.conv_wgrad([hseg], [(0, -1)], S * B, 1, T, 4 * H, dg, OutMap(T * G, 0, G),
                           dwhh[ws], dy_offset=ws * 4 * H)
        _scatter(dwhh, unpack_maps(("whh", S, H, Kh), lambda *ws: torch.cat([
            torch.cat([a, a.new_zeros(4 * H, Kh - H)], 1) for a in ws], 0),
            [(4 * H, H)] * S, Kh, dev), [pg.get(m.weight_hh_l0) for m in sets], acc)
        # W_ih / gate-bias gradients (the two input halves accumulate) and the input gradient
        dwih = _empty(wp.shape, dev)
        dbias = _empty((G,), dev)
        nxt = [_empty((B, T, H), dev) for _ in range(S)] if li > 0 else None
        Kin = D4 * Ch if li == 0 else H
        for half in range(S):
            if li == 0:
                segs, taps = in0[half]
            else:
                segs, taps = [Seg(lt["r_in"][half], 0, SegGeom(H, T * H, 0, H, 1, T))], [(0, 0)]
            ops.conv_wgrad(segs, taps, B, 1, T, G, dg[half], OutMap(T * G, 0, G), dwih,
                           dbias, accumulate=half == 1)
            gseg = [Seg(dg[half], 0, SegGeom(G, T * G, 0, G, 1, T))]
            wti = _tw(("ih_t", id(owner), li, Kin), wp, lambda: ops.pack_weight(
                wp[:, :Kin].t().contiguous().unsqueeze(1), G))
            if li == 0:
                ops.conv(gseg, [(0, 0)], B, 1, T, Kin, wti, None, g_in0,
                         OutMap(D4 * T * C6, 0, C6, T * C6, 1, Ch), out_offset=half * Ch,
                         accumulate=True)
            else:
                ops.conv(gseg, [(0, 0)], B, 1, T, H, wti, None, nxt[half], OutMap(T * H, 0, H),
                         mfma_only=True)
        D = R.weight_ih_l0.shape[1]
        if li == 0:  # layer 0's packed K order is (tap f, channel), the parameter's (channel, f)
            fn = lambda *ws: torch.cat(ws, 0).reshape(G, D // D4, D4).permute(0, 2, 1).reshape(G, D)  # noqa: E731
        else:
            fn = lambda *ws: torch.cat(ws, 0)  # noqa: E731
        _scatter(dwih, unpack_maps(("wih", S, li, H, D, D4), fn, [(4 * H, D)] * S,
                                   wp.shape[1], dev),
                 [pg.get(m.weight_ih_l0) for m in sets], acc)
        # bias_ih and bias_hh both receive the gate-bias gradient
        bmaps = unpack_maps(("lstm_b", S, H), lambda *bs: torch.cat(
            [bs[2 * k] + bs[2 * k + 1] for k in range(S)]).reshape(-1, 1), [(4 * H,)] * (2 * S), 1, dev)
        _scatter(dbias, bmaps, [pg.get(b) for m in sets for b in (m.bias_ih_l0, m.bias_hh_l0)], acc)
        d_out = nxt
