"""Streaming inference of asteroid's DCCRNet_mini (clskd.streaming.StreamingDCCRNet_mini: the
per-layer hop, replayed as a hipGraph; FusedStreamingDCCRNet_mini: clskd_stream_hop_mini, one
launch per hop) on the reference's trained checkpoint in eval mode.

The reference has no streaming path, so both engines are pinned by equality with the offline
eval-mode forward on the same clip — the fp32 CPU oracle ``oracle.asteroid_cpu.forward(sd, x,
train=False)`` and the HIP offline ``model(x)`` — at the bar tests/test_gpu_asteroid.py holds the
offline HIP forward to against that oracle: max |diff| <= 1e-4 x peak(ref).  Between the two
engines, hop by hop, the bar is the DCCRN engines' 2e-6 (tests/test_gpu_streaming.py, inputs of
peak <= 1) scaled by max(1, peak).  Inputs are slices of the fixture mixtures (peak about 0.3).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import asteroid_cpu as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = ["606", "1038", "1132"]
ORACLE_BAR = 1e-4   # x peak(ref): tests/test_gpu_asteroid.py:55
ENGINE_BAR = 2e-6   # x max(1, peak): tests/test_gpu_streaming.py:84


@functools.lru_cache(maxsize=None)
def _fx():
    return golden("asteroid_mini.npz")


@functools.lru_cache(maxsize=None)
def _model():
    from clskd.asteroid import DCCRNet_mini, load_conf
    return DCCRNet_mini.from_pretrained(load_conf(_fx())).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _clip(B, L, start=16000):
    rows = np.stack([A.mixture_from_wav(_fx()[i + "/mixture"])[start:start + L] for i in IDS[:B]])
    assert rows.shape == (B, L)
    return rows


@functools.lru_cache(maxsize=None)
def _oracle(B, L, start=16000):
    with torch.no_grad():
        ref = A.forward(A.state_dict_from_fixture(_fx()), torch.from_numpy(_clip(B, L, start)),
                        train=False).numpy()
    ref.setflags(write=False)
    return ref


def _engine(name, B):
    from clskd.streaming import FusedStreamingDCCRNet_mini, StreamingDCCRNet_mini
    if name == "fused":
        return FusedStreamingDCCRNet_mini(_model(), B)
    return StreamingDCCRNet_mini(_model(), B, graph=name == "graph")


def _dev(rows):
    return torch.from_numpy(rows).to(DEV)


@pytest.mark.parametrize("engine", ["graph", "fused"])
def test_process_matches_offline_eval_forward(engine):
    """B = 2, L = 3200 (29 frames, 32 input + 9 drain hops: every ring wraps, the graph is captured
    after the warm hops, the whole drain) against the CPU oracle and the HIP offline forward."""
    B, L = 2, 3200
    x = _dev(_clip(B, L))
    s = _engine(engine, B)
    out = s.process(x)
    torch.cuda.synchronize()
    assert out.shape == (B, L)
    ref = _oracle(B, L)
    with torch.no_grad():
        off = _model()(x)[:, 0].cpu().numpy()
    o = out.cpu().numpy()
    e_ref, e_off = np.abs(o - ref).max(), np.abs(o - off).max()
    peak = np.abs(ref).max()
    print(f"mini {engine} {B} x {L}: max |diff| oracle {e_ref:.2e} offline HIP {e_off:.2e} "
          f"(peak {peak:.3f}, bar {ORACLE_BAR * peak:.2e})")
    assert e_ref <= ORACLE_BAR * peak
    assert e_off <= ORACLE_BAR * np.abs(off).max()
    if engine == "graph":
        assert s.graph is not None, "steady-state hops must replay the captured graph"
        assert s.replays == L // 100 - s.CAPTURE_AFTER, s.replays


@pytest.mark.parametrize("L", [1000, 3250])
def test_fused_shortest_and_ragged_clip(L):
    """L = 1000: T = 7 frames, one LSTM frame, an output that is almost all drain.  L = 3250: the
    50 samples past the last complete hop are exactly zero (the offline pad_x_to_y)."""
    B = 2
    out = _engine("fused", B).process(_dev(_clip(B, L))).cpu().numpy()
    ref = _oracle(B, L)
    assert out.shape == ref.shape == (B, L)
    err, peak = np.abs(out - ref).max(), np.abs(ref).max()
    print(f"mini fused L={L}: max |diff| oracle {err:.2e} (peak {peak:.3f})")
    assert err <= ORACLE_BAR * peak
    if L % 100:
        assert np.all(out[:, L - L % 100:] == 0.0) and np.all(ref[:, L - L % 100:] == 0.0)


@pytest.mark.parametrize("B", [1, 3])
def test_fused_hop_matches_per_layer_hop(B):
    """clskd_stream_hop_mini against the per-layer hop, hop by hop through step() and finish():
    None for exactly the first 9 hops, then every block equal within 2e-6 x max(1, peak)."""
    L = 2400
    x = _dev(_clip(B, L))
    a, b = _engine("fused", B), _engine("eager", B)
    worst = 0.0
    for h in range(L // 100):
        ya, yb = a.step(x[:, h * 100:(h + 1) * 100]), b.step(x[:, h * 100:(h + 1) * 100])
        if h < 9:
            assert ya is None and yb is None, h
            continue
        assert ya is not None and yb is not None, h
        assert ya.shape == yb.shape == (B, 100)
        worst = max(worst, (ya - yb).abs().max().item())
    fa, fb = a.finish(), b.finish()
    assert fa.shape == fb.shape == (B, 900)
    worst = max(worst, (fa - fb).abs().max().item())
    peak = float(np.abs(_clip(B, L)).max())
    print(f"mini fused vs per-layer hop, B={B}: max |diff| {worst:.2e} (input peak {peak:.3f})")
    assert worst <= ENGINE_BAR * max(1.0, peak), worst


def test_fused_streams_are_independent():
    """One workgroup per stream, a K split that does not depend on B: a B = 3 run equals three
    B = 1 runs bit for bit."""
    L = 2400
    x = _dev(_clip(3, L))
    out3 = _engine("fused", 3).process(x)
    one = _engine("fused", 1)
    for j in range(3):
        assert torch.equal(out3[j:j + 1], one.process(x[j:j + 1])), j


@pytest.mark.parametrize("engine", ["eager", "fused"])
def test_reset_serves_clip_after_clip(engine):
    """process(A), reset(), process(B) is bit-identical to a fresh object on B."""
    B, L = 2, 2000
    xa, xb = _dev(_clip(B, L)), _dev(_clip(B, L, 24000))
    s = _engine(engine, B)
    s.process(xa)
    s.reset()
    got = s.process(xb)
    assert torch.equal(got, _engine(engine, B).process(xb))
    # and by hand: reset(), step() ..., finish()
    s.reset()
    outs = [s.step(xb[:, h * 100:(h + 1) * 100]) for h in range(L // 100)]
    outs = [y for y in outs if y is not None] + [s.finish()]
    assert torch.equal(torch.cat(outs, 1), got)


def test_invalid_use_raises_value_error():
    from clskd.asteroid import DCCRNet_mini, load_conf
    from clskd.streaming import FusedStreamingDCCRNet_mini, StreamingDCCRNet_mini
    train = DCCRNet_mini.from_pretrained(load_conf(_fx())).to(DEV)  # train mode, as constructed
    for cls in (StreamingDCCRNet_mini, FusedStreamingDCCRNet_mini):
        with pytest.raises(ValueError, match="eval"):
            cls(train, 1)
        s = cls(_model(), 2)
        with pytest.raises(ValueError, match="1000"):
            s.process(_dev(_clip(2, 900)))   # T = 6: no frame for the last encoder
        with pytest.raises(ValueError):
            s.process(_dev(_clip(3, 2000)))  # wrong batch size
        with pytest.raises(ValueError):
            s.step(_dev(_clip(3, 100)))
