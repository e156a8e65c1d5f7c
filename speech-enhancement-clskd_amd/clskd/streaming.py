"""Streaming DCCRN inference (config C5: 16 kHz, 25 ms window / 6.25 ms hop, hipGraph per hop).

The reference is offline only (``eval.py:47-60``); SURVEY.md §8 f rank 3 pins the streaming path
by equality with the offline eval-mode forward (``DCCRN.forward``, ``DCCRN.py:149-240``) on the
same input.  Per hop of 100 new samples (B streams in parallel):

* ConvSTFT of the newest 400-sample window (one framing GEMM row per stream);
* the encoder is causal in time (``F.pad(x, [1, 0])``, ``tools_for_model.py:237``): each layer keeps
  a 2-frame input window [t-1, t];
* the complex LSTMs carry (h, c) across hops (``clskd_lstm_cell``);
* each decoder layer looks ONE frame ahead (``ConvTranspose2d`` time kernel 2 + ``[..., 1:]``,
  ``DCCRN.py:201-206``), so layer d produces frame t-1-d at hop t from a 2-frame window of its
  input and its skip; the mask (and the enhanced frame) lags the input by ``LOOKAHEAD`` = 6 hops;
* mask 'E' + ConviSTFT frame + overlap-add over a 4-frame ring emits 100 final samples.

Output latency: 9 hops (900 samples = 56.25 ms): 6 decoder look-ahead frames + the 300-sample
STFT centring.  All per-hop buffers are time-major (``[slot][B][F][C]``) so each hop's newest
frame is one contiguous slot that kernels write directly; windows shift by slot copies.  The
steady-state hop (about 70 launches) is captured once as a hipGraph and replayed.

Eval-mode BatchNorm only (running statistics, as at inference).  Flush: after the last input
frame the decoder pipeline drains with zero frames (the offline decoder's out-of-range inputs).
"""
import torch

from . import clstm
from . import config as cfg
from . import ops
from .model import refuse_cbn, refuse_mask_mode, refuse_real_lstm
from .ops import OutMap, Seg, SegGeom

HOP, WIN = 100, 400
LOOKAHEAD = 6  # decoder frames: layer d reads its input one frame ahead, 6 layers (a DCCRN of
# another depth looks ahead by its own layer count: StreamingDCCRN.lookahead)
LATENCY_HOPS = LOOKAHEAD + 3  # + the 300-sample centring of the STFT framing


def _seg_tm(buf, slot0=0, nslots=None, c0=0, C=None):
    """Segment over a time-major window buf[S][B][F][Ct] (slots slot0.. as time)."""
    S, B, F, Ct = buf.shape
    C = Ct - c0 if C is None else C
    nslots = S - slot0 if nslots is None else nslots
    return Seg(buf, slot0 * B * F * Ct + c0, SegGeom(C, F * Ct, Ct, B * F * Ct, F, nslots))


class StreamingDCCRN:
    """Hop-by-hop DCCRN enhancement of B parallel streams with a captured hipGraph per hop.

    step(x_hop [B][100]) -> [B][100] enhanced samples, delayed by LATENCY_HOPS hops (None while
    the pipeline fills); finish() drains the look-ahead; process(x [B][L]) runs a whole clip and
    returns the offline-aligned [B][L] output (equal to model.eval()(x) up to fp32 rounding)."""

    def __init__(self, model, batch, graph=True):
        refuse_cbn(model, "StreamingDCCRN")
        refuse_real_lstm(model, "StreamingDCCRN")
        if model.training:
            raise ValueError("StreamingDCCRN runs eval-mode BatchNorm: call model.eval() first")
        self.m = model
        self.B = B = batch
        dev = next(model.parameters()).device
        self.dev = dev
        f32 = dict(device=dev, dtype=torch.float32)
        kn = model.kernel_num
        self.nl = nl = len(kn) - 1
        self.lookahead = nl  # one frame per decoder layer (LOOKAHEAD for the six-layer models)
        self.H = H = model.rnn_units // 2
        C6 = kn[-1]
        self.D4 = D4 = 256 // (2 ** nl)
        # ---- buffers (all zero: the causal / centring pads of the first frames)
        self.x_in = torch.zeros(B, HOP, **f32)
        self.wav_out = torch.zeros(B, HOP, **f32)
        self.xwin = torch.zeros(B, WIN, **f32)
        self.xtmp = torch.zeros(B, WIN - HOP, **f32)
        self.spec = torch.zeros(nl + 1, B, 514, **f32)            # spectra t-nl .. t
        self.spec_b = torch.zeros(B, 256, 1, 2, **f32)            # encoder-0 input frame (BFTC)
        Fi = [256 // (2 ** i) for i in range(nl + 1)]
        Cin = [2] + list(kn[1:-1])
        self.ewin = [torch.zeros(2, B, Fi[i], Cin[i], **f32) for i in range(nl)]   # enc inputs
        self.eraw = [torch.zeros(B, Fi[i + 1], 1, kn[i + 1], **f32) for i in range(nl)]
        # encoder output ring of depth nl + 1 - i: decoder layer nl - 1 - i reads frames
        # (t-nl+i, t-nl+1+i)
        self.ering = [torch.zeros(nl + 1 - i, B, Fi[i + 1], kn[i + 1], **f32) for i in range(nl)]
        self.gx = torch.zeros(2, B, 8 * H, **f32)
        self.h = torch.zeros(model.hidden_layers, 2, 2 * B, H, **f32)
        self.c = torch.zeros(model.hidden_layers, 2, 2 * B, H, **f32)
        self.hs = torch.zeros(2, 2 * B, H, **f32)
        self.rio = [(torch.zeros(B, H, **f32), torch.zeros(B, H, **f32))
                    for _ in range(model.hidden_layers)]
        # decoder input windows: d = 0 the LSTM projection (dec_in), d > 0 decoder d-1 output
        Fd = [D4 * (2 ** d) for d in range(nl)]
        Co = [model.decoder[d][0].out_channels * 2 for d in range(nl)]
        self.dwin = [torch.zeros(2, B, D4, C6, **f32)] + \
                    [torch.zeros(2, B, 2 * Fd[d - 1], Co[d - 1], **f32) for d in range(1, nl)]
        self.draw = [torch.zeros(B, 2 * Fd[d], 1, Co[d], **f32) for d in range(nl - 1)]
        self.mask = torch.zeros(B, 256, 2, 2, **f32)   # last decoder output at time slot 1
        self.est = torch.zeros(B, 1, 516, **f32)
        self.frames = torch.zeros(B, 4, WIN, **f32)     # OLA ring u-3 .. u
        self.ftmp = torch.zeros(B, 3, WIN, **f32)
        self.tmp = {}
        self.Fd, self.Co, self.Fi, self.Cin = Fd, Co, Fi, Cin
        # ---- eval-mode BatchNorm coefficients [scale | shift] (fixed at inference)
        self.ebn = [self._bn_coef(model.encoder[i][1]) for i in range(nl)]
        self.dbn = [self._bn_coef(model.decoder[d][1]) for d in range(nl - 1)]
        self.t = 0
        self.graph = None
        self.use_graph = graph
        self.steps_run = 0

    def _bn_coef(self, bn):
        x = torch.empty(1, bn.num_features, device=self.dev)
        return ops.batch_norm_bftc(x, None, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                   False, bn.momentum, bn.eps)

    def _bn_apply(self, x, y, coef, alpha):
        Cn = x.shape[-1]
        sc = coef.data_ptr()
        ops.check(ops.lib().clskd_bn_apply(x.data_ptr(), y.data_ptr(), x.numel() // Cn, Cn, sc,
                                           sc + 4 * Cn, ops.ptr(alpha), ops._dt(x), ops._stream()),
                  "bn_apply")

    def _shift(self, buf):
        """Time-major window: slot k <- slot k+1 for all but the newest slot."""
        S = buf.shape[0]
        if S == 2:
            buf[0].copy_(buf[1])
            return
        tmp = self.tmp.get(id(buf))
        if tmp is None:
            tmp = self.tmp[id(buf)] = torch.empty_like(buf[1:])
        tmp.copy_(buf[1:])
        buf[:-1].copy_(tmp)

    # ------------------------------------------------------------------------------------
    def _hop(self, live_in=True, zero_from=None):
        """One hop.  live_in=False (flush): no new input frame (encoder / LSTM frames are the
        offline out-of-range zeros); zero_from = T: decoder outputs of frames >= T are zero."""
        m, B, nl, H = self.m, self.B, self.nl, self.H
        from .model import DCCRN
        t = self.t
        # ---- shift every window / ring by one frame
        self.xtmp.copy_(self.xwin[:, HOP:])
        self.xwin[:, :WIN - HOP].copy_(self.xtmp)
        self.xwin[:, WIN - HOP:].copy_(self.x_in)
        self._shift(self.spec)
        for w in self.ewin + self.ering + self.dwin:
            self._shift(w)
        self.ftmp.copy_(self.frames[:, 1:])
        self.frames[:, :3].copy_(self.ftmp)
        if live_in:
            # ---- ConvSTFT of the newest window (tools_for_model.py:53-67)
            ops.conv([Seg(self.xwin, 0, SegGeom(HOP, WIN, 0, HOP, 1, 4))],
                     [(0, kt) for kt in range(4)], B, 1, 1, 514, m._stft_w(), None, self.spec[-1],
                     OutMap(514, 0, 514))
            ops.spec_bftc(self.spec[-1].view(B, 1, 514), 1, 258, 256, self.spec_b)
            self.ewin[0][1].copy_(self.spec_b.view(B, 256, 2))
            # ---- encoder (DCCRN.py:171-176): window [t-1, t], taps (kf-2, kt)
            for i in range(nl):
                wp, bias = m._enc_w(i, "fp32")
                Fo, Co = self.Fi[i + 1], m.kernel_num[i + 1]
                ops.conv([_seg_tm(self.ewin[i])], [(kf - 2, kt) for kf in range(5) for kt in range(2)],
                         B, Fo, 1, Co, wp, bias, self.eraw[i], OutMap(Fo * Co, Co, Co), stride_f=2)
                bn, pr = m.encoder[i][1], m.encoder[i][2]
                dst = self.ewin[i + 1][1] if i + 1 < nl else self.ering[i][-1]
                self._bn_apply(self.eraw[i].view(B, Fo, Co), dst, self.ebn[i], pr.weight)
                if i + 1 < nl:
                    self.ering[i][-1].copy_(dst)
            # ---- complex LSTMs (DCCRN.py:178-199), state carried across hops
            C6, Ch, D4 = m.kernel_num[-1], m.kernel_num[-1] // 2, self.D4
            in0 = [([_seg_tm(self.ering[nl - 1], 1, 1, half * Ch, Ch)], [(f, 0) for f in range(D4)])
                   for half in range(2)]  # newest frame (slot 1) of the last encoder output's ring
            r_in = clstm.hop(in0, lambda li, segs: m._lstm_w(li, "fp32")[:3], m.hidden_layers, B, H,
                             self.gx, self.h, self.c, self.hs, self.rio)
            last = m.enhance[m.hidden_layers - 1]
            packs = m._lstm_w(m.hidden_layers - 1, "fp32")
            for half in range(2):
                ops.conv([Seg(r_in[half], 0, SegGeom(H, H, 0, H, 1, 1))], [(0, 0)], B, 1, 1,
                         last.projection_dim, packs[3 + 2 * half], packs[4 + 2 * half], self.dwin[0][1],
                         OutMap(D4 * C6, 0, 0, 1, C6, D4), out_offset=half * Ch)
        else:
            for r in self.ering:
                r[-1].zero_()
            self.dwin[0][1].zero_()
        # ---- decoder (DCCRN.py:201-206): layer d emits frame t-1-d from [t-1-d, t-d]
        for d in range(nl):
            F, Co = self.Fd[d], self.Co[d]
            ring = self.ering[nl - 1 - d]   # depth d + 2: slots 0, 1 = frames t-1-d, t-d
            Cof, Csk = self.dwin[d].shape[-1], ring.shape[-1]
            last_layer = d == nl - 1
            out_frame = t - 1 - d
            dead = zero_from is not None and out_frame >= zero_from
            dst = self.mask if last_layer else self.draw[d]
            if dead:
                if last_layer:
                    self.mask[:, :, 1].zero_()
                else:
                    self.dwin[d + 1][1].zero_()
                continue
            segs = [_seg_tm(self.dwin[d], 0, 2), _seg_tm(ring, 0, 2)]
            for parity in (0, 1):
                taps = [(dF, 1 - kt) for _, dF in DCCRN._DEC_TAPS[parity] for kt in (0, 1)]
                wp, bias = m._dec_w(d, parity, "fp32")
                if last_layer:  # mask [B][256][2][2], written at time slot 1
                    omap, off = OutMap(256 * 2 * 2, 2 * 2, 2, of_mul=2, of_add=parity), 2
                else:
                    omap, off = OutMap(2 * F * Co, Co, Co, of_mul=2, of_add=parity), 0
                ops.conv(segs, taps, B, F, 1, Co, wp, bias, dst, omap, out_offset=off)
            if not last_layer:
                pr = m.decoder[d][2]
                self._bn_apply(self.draw[d].view(B, 2 * F, Co), self.dwin[d + 1][1], self.dbn[d],
                               pr.weight)
        # ---- mask 'E' / 'C' / 'R' on frame t-nl, ConviSTFT frame, overlap-add (DCCRN.py:207-237)
        ops.mask(m.masking_mode, self.spec[0].view(B, 1, 514), self.mask, 1, self.est)
        winv, window = m._istft_w()
        ops.conv([Seg(self.est, 0, SegGeom(516, 516, 0, 516, 1, 1))], [(0, 0)], B, 1, 1, WIN, winv,
                 None, self.frames, OutMap(4 * WIN, 0, 0), out_offset=3 * WIN)
        ops.ola_hop(self.frames, window, HOP, HOP, 300, True, self.wav_out)
        self.t += 1

    def _capture(self):
        """Capture the steady-state hop once its kernels' launch plans exist (warm hops)."""
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        snap = self._snapshot()
        with torch.cuda.graph(g, stream=ops.capture_stream(self.dev)):
            self._hop()
        self._restore(snap)   # capture only records: the hop counter must not advance
        self.graph = g

    def _snapshot(self):
        return self.t

    def _restore(self, t):
        self.t = t

    def step(self, x_hop):
        """Feed 100 new samples per stream; returns the enhanced hop 9 hops behind (or None)."""
        self.x_in.copy_(x_hop)
        if self.graph is None and self.use_graph and self.steps_run >= 2:
            self._capture()
        if self.graph is not None:
            self.graph.replay()
            self.t += 1
        else:
            self._hop()
        self.steps_run += 1
        return self.wav_out.clone() if self.t - 1 - self.lookahead >= 3 else None

    def process(self, x):
        """Whole clip x [B][L] (L % 100 == 0) through the hop loop + flush -> [B][L], aligned
        with the offline forward's output."""
        B, L = x.shape
        assert B == self.B and L % HOP == 0
        T = cfg.n_frames(L)
        outs = []
        for t in range(T):
            s = t * HOP
            hop = x[:, s:s + HOP] if s + HOP <= L else torch.zeros(B, HOP, device=x.device)
            y = self.step(hop)
            if y is not None:
                outs.append(y)
        for _ in range(self.lookahead):   # drain the decoder look-ahead with zero frames (eager)
            self.x_in.zero_()
            self._hop(live_in=False, zero_from=T)
            outs.append(self.wav_out.clone())
        return torch.cat(outs, 1)[:, :L]


class FusedStreamingDCCRN(StreamingDCCRN):
    """The same hop as StreamingDCCRN, as ONE launch per hop (clskd_stream_hop,
    csrc/stream_hop.hip): one workgroup per stream walks the ConvSTFT row, encoder, complex
    LSTMs, projection, decoder, mask 'E', iSTFT row and overlap-add with each layer's current
    frame in LDS and the frames the causal convolutions / decoder look-ahead need in per-stream
    rings.  Same step() / process() contract and latency (9 hops); the ~70-launch hop becomes one
    launch, so the hop is no longer bound by launch and dependency latency.  Weights are the
    offline forward's packed fp32 operands in the kernel's k-quad layout [K/4][N][4] (built once;
    re-create the object after changing the model's parameters)."""

    def __init__(self, model, batch):
        refuse_mask_mode(model, "FusedStreamingDCCRN (mask 'E' is compiled into its hop kernel)")
        super().__init__(model, batch, graph=False)
        m, B, dev = self.m, self.B, self.dev
        from . import _lib
        nl, H, D4 = self.nl, self.H, self.D4
        if nl != 6 or m.hidden_layers != 2:
            raise NotImplementedError("the fused hop is built for the 6-layer, 2-LSTM DCCRN")
        kn = m.kernel_num
        if any(c & (c - 1) for c in kn[1:]):
            # csrc/stream_hop.hip deals each layer's outputs to lanes by shifts and masks of the
            # channel count: it checks this at the first launch; say it here, by name
            raise NotImplementedError(
                f"the fused hop is built for power-of-two widths, not kernel_num={kn[1:]}")
        C6 = kn[-1]
        keep = []

        def q4(w, K, ci=None):
            """packed [N][Kp] (first K columns real) -> k-quad [K/4][N][4]; ci: pad each tap's ci
            input channels to a quad (encoder 0's (re, im))."""
            w = w.float()[:, :K]
            N = w.shape[0]
            if ci is not None:
                w = torch.nn.functional.pad(w.reshape(N, K // ci, ci), (0, 4 - ci)).reshape(N, -1)
                K = w.shape[1]
            assert K % 4 == 0, K
            t = w.reshape(N, K // 4, 4).permute(1, 0, 2).contiguous()
            keep.append(t)
            return t.data_ptr()

        def p(t):
            keep.append(t)
            return t.data_ptr()

        a = _lib.StreamHopArgs()
        a.stft_w = q4(m._stft_w(), WIN)
        winv, window = m._istft_w()
        a.istft_w, a.window = q4(winv, 516), p(window)
        for i in range(nl):
            wp, bias = m._enc_w(i, "fp32")
            a.enc_w[i], a.enc_b[i] = q4(wp, 10 * kn[i], ci=2 if i == 0 else None), p(bias)
            a.enc_coef[i], a.enc_alpha[i] = p(self.ebn[i]), p(m.encoder[i][2].weight.detach().float())
            a.enc_cin[i], a.enc_cout[i] = kn[i], kn[i + 1]
        for li in range(2):
            packs = m._lstm_w(li, "fp32")
            K = D4 * (C6 // 2) if li == 0 else H
            whh = packs[2].float().reshape(8 * H, H)  # [2][4H][H] -> n = ws*4H + g
            a.lstm_w[li], a.lstm_b[li], a.lstm_whh[li] = q4(packs[0], K), p(packs[1]), q4(whh, H)
            if li == 1:
                for half in range(2):
                    a.proj_w[half], a.proj_b[half] = q4(packs[3 + 2 * half], H), p(packs[4 + 2 * half])
        for d in range(nl):
            for parity in (0, 1):
                wp, bias = m._dec_w(d, parity, "fp32")
                ci = (C6 if d == 0 else self.Co[d - 1]) + kn[nl - d]
                a.dec_w[d][parity], a.dec_b[d][parity] = q4(wp, (6 if parity == 0 else 4) * ci), p(bias)
            if d < nl - 1:
                a.dec_coef[d], a.dec_alpha[d] = p(self.dbn[d]), p(m.decoder[d][2].weight.detach().float())
            a.dec_ca[d] = C6 if d == 0 else self.Co[d - 1]
            a.dec_cb[d] = kn[nl - d]
            a.dec_co[d] = self.Co[d]
        a.H, a.D4, a.B = H, D4, B
        # per-stream state layout (floats)
        off = 0

        def take(n):
            nonlocal off
            o = off
            off += (n + 3) // 4 * 4
            return o

        a.off_xwin = take(WIN)
        a.off_spec = take(7 * 514)
        for i in range(nl):
            a.off_enc[i] = take((7 - i) * (128 >> i) * kn[i + 1])
        a.off_decin = take(2 * D4 * C6)
        for d in range(nl - 1):
            a.off_dout[d] = take(2 * 2 * self.Fd[d] * self.Co[d])
        a.off_h = take(2 * 4 * H)
        a.off_c = take(2 * 4 * H)
        a.off_frames = take(4 * WIN)
        a.state_stride = off
        self.fstate = torch.zeros(B, off, device=dev, dtype=torch.float32)
        a.state = self.fstate.data_ptr()
        a.x_in, a.wav_out = self.x_in.data_ptr(), self.wav_out.data_ptr()
        self._args, self._keep = a, keep

    def _hop(self, live_in=True, zero_from=None):
        a = self._args
        a.t, a.live = self.t, int(live_in)
        a.zero_from = -1 if zero_from is None else int(zero_from)
        ops.check(ops.lib().clskd_stream_hop(a, ops._stream()), "stream_hop")
        self.t += 1

    def step(self, x_hop):
        self.x_in.copy_(x_hop)
        self._hop()
        self.steps_run += 1
        return self.wav_out.clone() if self.t - 1 - LOOKAHEAD >= 3 else None


# ======================================================================================
# asteroid DCCRNet_mini ('DCCRN-CL-test', clskd.asteroid): the distilled student the reference
# checkpoints and evaluates, hop by hop
# ======================================================================================
MINI_LOOKAHEAD = 6                    # the six encoder blocks read one frame ahead each
MINI_LATENCY_HOPS = MINI_LOOKAHEAD + 3  # + the 3 hops that complete an uncentred 400-sample frame
MINI_MIN_SAMPLES = (MINI_LATENCY_HOPS + 1) * HOP


class _StreamingMini:
    """step() / finish() / process() / reset() of the two DCCRNet_mini streaming engines.

    Time structure (oracle/asteroid_cpu.py:85-138, eval-mode BatchNorm).  Hop h brings samples
    [100h, 100h + 100); frame u covers [100u, 100u + 400) (no centring), so it is complete after
    hop u + 3.  Encoder block i reads its input at frames t and t + 1 and therefore emits frame
    u - (i + 1) when frame u arrives; the LSTMs (carried state), the Linear, the five transposed
    convs and the output layer are causal and emit frame u - 6; the mask of frame u - 6 times
    spectrum frame u - 6 enters a 4-frame plain overlap-add that completes output block u - 6.
    Input hop h yields output block h - 9: 9 hops = 56.25 ms of algorithmic latency.

    Frames the offline forward does not have are zeros wherever a later layer reads them
    (BatchNorm + PReLU of a zero row is not zero, and the output layer has a bias): every frame
    before frame 0, and after the last input hop (T frames in all) the spectrum, the encoders and
    the LSTM / Linear at once, transposed conv d (0..5) from drain hop d + 2 on.

    Equal to ``model.eval()(x)``: running statistics.  A train-mode forward (what the reference's
    eval.py runs) normalises with the statistics of the whole utterance and cannot be streamed.
    Weights are packed once at construction: re-create the object after the parameters change."""

    def __init__(self, model, batch):
        if model.training:
            raise ValueError(f"{type(self).__name__} runs eval-mode BatchNorm (running statistics): "
                             "call model.eval() first")
        self.m = model
        self.B = int(batch)
        self.dev = next(model.parameters()).device
        mk = model.masker
        self.encs = list(mk.encoders[:-1])
        self.decs = [(blk.deconv, blk) for blk in list(mk.decoders)[1:]] + [(mk.output_layer[0], None)]
        self.rnn = mk.encoders[-1].rnn
        if len(self.encs) != 6 or len(self.decs) != 6 or len(self.rnn.rnns) != 2:
            raise NotImplementedError("built for the 6-block, 2-LSTM DCCRNet_mini")
        self.H = self.rnn.rnns[0].re_module.rnn.hidden_size
        self.Cin = [2 * e.conv.re_module.in_channels for e in self.encs]    # (re | im) channels
        self.Cenc = [2 * e.conv.re_module.out_channels for e in self.encs]
        self.Fenc = [128 >> i for i in range(6)]                             # encoder output bins
        self.D4, self.C6 = self.Fenc[5], self.Cenc[5]
        self.Fd = [self.D4 << d for d in range(6)]                           # transposed-conv input bins
        self.Co = [2 * dc.re_module.out_channels for dc, _ in self.decs]
        self.Ca = [self.C6] + self.Co[:-1]
        self.t = 0
        self.steps_run = 0

    # ---- eval-mode BatchNorm of the (re | im) channels as [scale | shift], the two PReLU slopes
    def _bn_coef(self, blk):
        nr, ni = blk.norm.re_module, blk.norm.im_module
        with torch.no_grad():
            g, b, rm, rv = (torch.cat([getattr(nr, k), getattr(ni, k)]).float().contiguous()
                            for k in ("weight", "bias", "running_mean", "running_var"))
            x = torch.empty(1, g.numel(), device=self.dev)
            coef = ops.batch_norm_bftc(x, None, g, b, rm, rv, False, nr.momentum, nr.eps)
            alpha = torch.cat([blk.activation.re_module.weight,
                               blk.activation.im_module.weight]).float().contiguous()
        return coef, alpha

    def _zero_state(self):
        raise NotImplementedError

    def _hop(self, live, drain):
        raise NotImplementedError

    def reset(self):
        """Back to the start of a stream: zero state, hop counter 0 (one object, clip after clip)."""
        self._zero_state()
        self.t = 0

    def _check_hop(self, x_hop):
        if tuple(x_hop.shape) != (self.B, HOP):
            raise ValueError(f"expected a hop of shape ({self.B}, {HOP}), got {tuple(x_hop.shape)}")

    def step(self, x_hop):
        """Feed 100 new samples per stream; returns the enhanced block 9 hops behind (None for the
        first 9 hops)."""
        self._check_hop(x_hop)
        self.x_in.copy_(x_hop)
        self._hop(True, 0)
        self.steps_run += 1
        return self.wav_out.clone() if self.t > MINI_LATENCY_HOPS else None

    def finish(self):
        """End of the stream: the 9 drain hops -> [B][900], the last 9 blocks of the clip (6 hops
        empty the transposed convs, 3 flush the overlap-add).  reset() starts the next clip."""
        if self.t < MINI_LATENCY_HOPS + 1:
            raise ValueError(f"a clip needs at least {MINI_MIN_SAMPLES} samples (7 frames: one for "
                             f"the last encoder), got {self.t * HOP}")
        outs = []
        for k in range(1, MINI_LATENCY_HOPS + 1):
            self._hop(False, k)
            outs.append(self.wav_out.clone())
        return torch.cat(outs, 1)

    def process(self, x):
        """Whole clip x [B][L] -> [B][L], equal to the offline eval-mode forward: the complete
        hops, the drain, zeros for the L % 100 samples the offline model pads (pad_x_to_y)."""
        if x.dim() != 2 or x.shape[0] != self.B:
            raise ValueError(f"expected [{self.B}][L] input, got {tuple(x.shape)}")
        L = x.shape[1]
        if L < MINI_MIN_SAMPLES:
            raise ValueError(f"a clip needs at least {MINI_MIN_SAMPLES} samples (7 frames: one for "
                             f"the last encoder), got {L}")
        self.reset()
        outs = []
        for h in range(L // HOP):
            y = self.step(x[:, h * HOP:(h + 1) * HOP])
            if y is not None:
                outs.append(y)
        outs.append(self.finish())
        if L % HOP:
            outs.append(torch.zeros(self.B, L % HOP, device=x.device, dtype=torch.float32))
        return torch.cat(outs, 1)


class StreamingDCCRNet_mini(_StreamingMini):
    """DCCRNet_mini hop by hop with the library's per-layer kernels (about 60 launches per hop),
    the steady-state hop captured once as a hipGraph and replayed (graph=True): the second,
    independent implementation the fused hop is checked against.  See _StreamingMini for the
    contract and the time structure.  Buffers are time-major windows [slot][B][F][C], oldest
    slot first, shifted by one slot per hop."""

    CAPTURE_AFTER = MINI_LATENCY_HOPS + 2  # eager hops first: every launch plan of a full hop exists

    def __init__(self, model, batch, graph=True):
        super().__init__(model, batch)
        m, B, H, D4, C6 = self.m, self.B, self.H, self.D4, self.C6
        f32 = dict(device=self.dev, dtype=torch.float32)
        z = lambda *shape: torch.zeros(*shape, **f32)  # noqa: E731
        self.x_in, self.wav_out = z(B, HOP), z(B, HOP)
        self.xwin, self.xtmp = z(B, WIN), z(B, WIN - HOP)
        self.spec = z(MINI_LOOKAHEAD + 1, B, 514)          # spectrum frames u-6 .. u
        self.spec_b = z(B, 256, 1, 2)
        Fin = [256 >> i for i in range(6)]
        self.ewin = [z(2, B, Fin[i], self.Cin[i]) for i in range(6)]       # encoder i input: u-i-1, u-i
        self.eraw = [z(B, self.Fenc[i], 1, self.Cenc[i]) for i in range(6)]
        # encoder i output ring: frames u-7 .. u-i-1 (slots 0, 1 = the skip of transposed conv 5-i)
        self.ering = [z(7 - i, B, self.Fenc[i], self.Cenc[i]) for i in range(6)]
        self.gx = z(2, B, 8 * H)
        self.h, self.c = z(2, 2, 2 * B, H), z(2, 2, 2 * B, H)
        self.hs = z(2, 2 * B, H)
        self.rio = [(z(B, H), z(B, H)) for _ in range(2)]
        self.dwin = [z(2, B, self.Fd[d], self.Ca[d]) for d in range(6)]    # transposed conv d input: u-7, u-6
        self.draw = [z(B, 2 * self.Fd[d], 1, self.Co[d]) for d in range(5)]
        self.mask = z(B, 256, 1, 2)
        self.est = z(B, 1, 516)
        self.frames, self.ftmp = z(B, 4, WIN), z(B, 3, WIN)               # synthesis frames u-9 .. u-6
        self._state = ([self.x_in, self.wav_out, self.xwin, self.spec, self.h, self.c, self.mask,
                        self.frames] + self.ewin + self.ering + self.dwin)
        self.tmp = {}
        # ---- operands, packed once
        with torch.no_grad():
            self.w_fb = m._fb_w()
            self.w_enc = [m._enc_w(i) for i in range(6)]
            self.w_lstm = [m._lstm_w(li) for li in range(2)]
            self.w_lin = m._lin_w()
            self.w_dec = [[m._dec_w(dc, parity, self.Ca[d] // 2) for parity in (0, 1)]
                          for d, (dc, _) in enumerate(self.decs)]
        self.ebn = [self._bn_coef(e) for e in self.encs]
        self.dbn = [self._bn_coef(blk) for _, blk in self.decs[:-1]]
        self.graph = None
        self._scope = None
        self.use_graph = graph
        self.replays = 0

    def _zero_state(self):
        for t in self._state:
            t.zero_()

    _shift = StreamingDCCRN._shift

    def _bn_apply(self, x, y, bn):
        coef, alpha = bn
        Cn = x.shape[-1]
        sc = coef.data_ptr()
        ops.check(ops.lib().clskd_bn_apply_reim(x.data_ptr(), y.data_ptr(), x.numel() // Cn, Cn, sc,
                                                sc + 4 * Cn, alpha.data_ptr(), ops._dt(x),
                                                ops._stream()), "bn_apply_reim")

    def _body(self, u, live, drain):
        """One hop whose newest frame is u (drain: the drain hop 1.., else 0)."""
        from .asteroid import DCCRNet_mini
        B, H, D4, C6 = self.B, self.H, self.D4, self.C6
        Ch = C6 // 2
        # ---- shift every window / ring by one frame
        self.xtmp.copy_(self.xwin[:, HOP:])
        self.xwin[:, :WIN - HOP].copy_(self.xtmp)
        if live:
            self.xwin[:, WIN - HOP:].copy_(self.x_in)
        else:
            self.xwin[:, WIN - HOP:].zero_()
        for w in [self.spec] + self.ewin + self.ering + self.dwin:
            self._shift(w)
        self.ftmp.copy_(self.frames[:, 1:])
        self.frames[:, :3].copy_(self.ftmp)
        # ---- STFTFB analysis of the newest window; Nyquist bin dropped (asteroid.py:301-305)
        if live and u >= 0:
            ops.conv([Seg(self.xwin, 0, SegGeom(HOP, WIN, 0, HOP, 1, 4))],
                     [(0, kt) for kt in range(4)], B, 1, 1, 514, self.w_fb[0], None, self.spec[-1],
                     OutMap(514, 0, 514))
            ops.spec_bftc(self.spec[-1].view(B, 1, 514), 0, 257, 256, self.spec_b)
            self.ewin[0][1].copy_(self.spec_b.view(B, 256, 2))
        else:
            self.spec[-1].zero_()
            self.ewin[0][1].zero_()
        # ---- encoders: block i emits frame u-i-1 from its input's frames (u-i-1, u-i)
        for i in range(6):
            Fo, Co = self.Fenc[i], self.Cenc[i]
            dsts = [self.ering[i][-1]] + ([self.ewin[i + 1][1]] if i < 5 else [])
            if live and u >= i + 1:
                ops.conv([_seg_tm(self.ewin[i])], [(kf - 2, kt) for kf in range(5) for kt in range(2)],
                         B, Fo, 1, Co, self.w_enc[i], None, self.eraw[i], OutMap(Fo * Co, Co, Co),
                         stride_f=2)
                self._bn_apply(self.eraw[i].view(B, Fo, Co), dsts[0], self.ebn[i])
                for dst in dsts[1:]:
                    dst.copy_(dsts[0])
            else:
                for dst in dsts:
                    dst.zero_()
        # ---- complex LSTMs on frame u-6 (carried state), complex Linear -> transposed conv 0 input
        if live and u >= MINI_LOOKAHEAD:
            in0 = [([_seg_tm(self.ering[5], 1, 1, half * Ch, Ch)], [(f, 0) for f in range(D4)])
                   for half in range(2)]
            r_in = clstm.hop(in0, lambda li, segs: self.w_lstm[li], 2, B, H, self.gx, self.h, self.c,
                             self.hs, self.rio)
            wre, bre, wim, bim = self.w_lin
            segs = [Seg(r_in[h], 0, SegGeom(H, H, 0, H, 1, 1)) for h in range(2)]
            for half, (w, b) in enumerate(((wre, bre), (wim, bim))):
                ops.conv(segs, [(0, 0)], B, 1, 1, Ch * D4, w, b, self.dwin[0][1],
                         OutMap(D4 * C6, 0, 0, 1, C6, D4), out_offset=half * Ch)
        else:
            self.dwin[0][1].zero_()
        # ---- transposed convs (the output layer last): frame u-6 from frames (u-7, u-6)
        for d in range(6):
            F, Co = self.Fd[d], self.Co[d]
            last = d == 5
            dst = self.mask if last else self.dwin[d + 1][1]
            if not (u >= MINI_LOOKAHEAD and drain <= d + 1):
                dst.zero_()
                continue
            segs = [_seg_tm(self.dwin[d], 0, 2), _seg_tm(self.ering[5 - d], 0, 2)]
            raw = self.mask if last else self.draw[d]
            for parity in (0, 1):
                taps = [(dF, 1 - kt) for _, dF in DCCRNet_mini._DEC_TAPS[parity] for kt in (0, 1)]
                wp, bias = self.w_dec[d][parity]
                ops.conv(segs, taps, B, F, 1, Co, wp, bias, raw,
                         OutMap(2 * F * Co, Co, Co, of_mul=2, of_add=parity))
            if not last:
                self._bn_apply(self.draw[d].view(B, 2 * F, Co), dst, self.dbn[d])
        # ---- bounded mask times spectrum frame u-6, synthesis row, plain overlap-add
        ops.check(ops.lib().clskd_mask_bdt(self.spec[0].data_ptr(), 514, self.mask.data_ptr(), 1, B, 1,
                                           self.est.data_ptr(), 516, ops._stream()), "mask_bdt")
        ops.conv([Seg(self.est, 0, SegGeom(516, 516, 0, 516, 1, 1))], [(0, 0)], B, 1, 1, WIN,
                 self.w_fb[1], None, self.frames, OutMap(4 * WIN, 0, 0), out_offset=3 * WIN)
        ops.ola_hop(self.frames, None, HOP, HOP, WIN - HOP, False, self.wav_out)

    def _capture(self):
        """Capture the steady-state hop (every frame exists) inside a CaptureScope, so the graph
        owns the stream-K workspaces of its conv launches."""
        torch.cuda.synchronize(self.dev)
        s = ops.capture_stream(self.dev)
        g = torch.cuda.CUDAGraph()
        self._scope = ops.CaptureScope([s])
        try:
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"), torch.no_grad():
                self._body(MINI_LOOKAHEAD, True, 0)  # recorded, not run: the state does not advance
        finally:
            self._scope.end()
        self.graph = g

    def _hop(self, live, drain):
        u = self.t - 3
        steady = live and u >= MINI_LOOKAHEAD
        if steady and self.use_graph and self.graph is None and self.steps_run >= self.CAPTURE_AFTER:
            self._capture()
        if steady and self.graph is not None:
            self.graph.replay()
            self.replays += 1
        else:
            with torch.no_grad():
                self._body(u, live, drain)
        self.t += 1


class FusedStreamingDCCRNet_mini(_StreamingMini):
    """DCCRNet_mini hop by hop as ONE launch per hop (clskd_stream_hop_mini,
    csrc/stream_hop_mini.hip): one workgroup per stream walks the analysis row, the encoders, the
    complex LSTMs, the Linear, the transposed convs, the bounded mask, the synthesis row and the
    overlap-add with each layer's current frame in LDS and the older frames in per-stream rings.
    Same step() / finish() / process() / reset() contract and latency (9 hops) as
    StreamingDCCRNet_mini.  Weights are fp32 copies in the kernel's k-quad layout [K/4][N][4],
    built once: re-create the object after changing the model's parameters."""

    def __init__(self, model, batch):
        super().__init__(model, batch)
        from . import _lib
        m, B, dev, H, D4, C6 = self.m, self.B, self.dev, self.H, self.D4, self.C6
        f32 = dict(device=dev, dtype=torch.float32)
        self.x_in, self.wav_out = torch.zeros(B, HOP, **f32), torch.zeros(B, HOP, **f32)
        keep = []

        def q4(w, K, ci=None):
            """packed [N][Kp] (first K columns real) -> k-quad [K/4][N][4]; ci: pad each tap's ci
            input channels to a quad (encoder 0's (re, im))."""
            w = w.float()[:, :K]
            N = w.shape[0]
            if ci is not None:
                w = torch.nn.functional.pad(w.reshape(N, K // ci, ci), (0, 4 - ci)).reshape(N, -1)
                K = w.shape[1]
            assert K % 4 == 0, K
            t = w.reshape(N, K // 4, 4).permute(1, 0, 2).contiguous()
            keep.append(t)
            return t.data_ptr()

        def p(t):
            t = t.detach().float().contiguous()
            keep.append(t)
            return t.data_ptr()

        a = _lib.StreamHopMiniArgs()
        with torch.no_grad():
            wa, ws = m._fb_w()
            a.stft_w, a.istft_w = q4(wa, WIN), q4(ws, 516)
            for i, e in enumerate(self.encs):
                a.enc_w[i] = q4(m._enc_w(i), 10 * self.Cin[i], ci=2 if i == 0 else None)
                coef, alpha = self._bn_coef(e)
                a.enc_coef[i], a.enc_alpha[i] = p(coef), p(alpha)
                a.enc_cin[i], a.enc_cout[i] = self.Cin[i], self.Cenc[i]
            for li in range(2):
                wp, bias, whh = m._lstm_w(li)
                K = D4 * (C6 // 2) if li == 0 else H
                a.lstm_w[li], a.lstm_b[li] = q4(wp, K), p(bias)
                a.lstm_whh[li] = q4(whh.float().reshape(8 * H, H), H)
            wre, bre, wim, bim = m._lin_w()
            a.lin_w = q4(torch.cat([wre[:, :2 * H], wim[:, :2 * H]], 0), 2 * H)
            a.lin_b = p(torch.cat([bre, bim]))
            for d, (dc, blk) in enumerate(self.decs):
                Cb = self.Cenc[5 - d]
                for parity in (0, 1):
                    wp, bias = m._dec_w(dc, parity, self.Ca[d] // 2)
                    a.dec_w[d][parity] = q4(wp, (6 if parity == 0 else 4) * (self.Ca[d] + Cb))
                    a.dec_b[d][parity] = p(bias) if bias is not None else None
                if blk is not None:
                    coef, alpha = self._bn_coef(blk)
                    a.dec_coef[d], a.dec_alpha[d] = p(coef), p(alpha)
                a.dec_ca[d], a.dec_cb[d], a.dec_co[d] = self.Ca[d], Cb, self.Co[d]
        a.H, a.D4, a.B = H, D4, B
        # per-stream state layout (floats)
        off = 0

        def take(n):
            nonlocal off
            o = off
            off += (n + 3) // 4 * 4
            return o

        a.off_xwin = take(WIN)
        a.off_spec = take(7 * 514)
        for i in range(6):
            a.off_enc[i] = take((7 - i) * self.Fenc[i] * self.Cenc[i])
        a.off_decin = take(2 * D4 * C6)
        for d in range(5):
            a.off_dout[d] = take(2 * 2 * self.Fd[d] * self.Co[d])
        a.off_h = take(2 * 4 * H)
        a.off_c = take(2 * 4 * H)
        a.off_frames = take(4 * WIN)
        a.state_stride = off
        self.fstate = torch.zeros(B, off, **f32)
        a.state = self.fstate.data_ptr()
        a.x_in, a.wav_out = self.x_in.data_ptr(), self.wav_out.data_ptr()
        self._args, self._keep = a, keep

    def _zero_state(self):
        self.fstate.zero_()
        self.x_in.zero_()
        self.wav_out.zero_()

    def _hop(self, live, drain):
        a = self._args
        a.t, a.live, a.drain = self.t, int(live), int(drain)
        ops.check(ops.lib().clskd_stream_hop_mini(a, ops._stream()), "stream_hop_mini")
        self.t += 1
