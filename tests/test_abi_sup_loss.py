"""CPU: the entries of csrc/sup_loss.hip validate their arguments before any launch — null
pointers, B = 0, L = 0 / T = 0, a row pitch under 514, a misaligned workspace come back as a status
code with a clskd_last_error text (no GPU compute is called) — and the workspace size queries are
monotone and bounded."""
import ctypes as C

from clskd import _lib

FAKE = 1 << 20  # never dereferenced: validation fails first
W5 = (C.c_float * 5)(1, 0, 0, 0, 0)


def _wave(lib, s=FAKE, y=FAKE, B=2, L=100, lds=100, ldy=100, w=W5, work=FAKE, out=FAKE, coef=FAKE):
    return lib.clskd_wave_loss(s, lds, y, ldy, B, L, w, 1.0, work, out, coef, None)


def test_wave_loss_rejects_bad_arguments():
    lib = _lib.load(require_gpu=False)
    assert _wave(lib, s=None) == -4 and b"wave_loss: null pointer" in lib.clskd_last_error()
    assert _wave(lib, y=None) == -4
    assert _wave(lib, w=None) == -4
    assert _wave(lib, work=None) == -4
    assert _wave(lib, out=None) == -4
    assert _wave(lib, B=0) < 0 and b"B=0" in lib.clskd_last_error()
    assert _wave(lib, B=65536) < 0
    assert _wave(lib, L=0) < 0 and b"L=0" in lib.clskd_last_error()
    assert _wave(lib, lds=99) < 0 and b"row strides" in lib.clskd_last_error()
    assert _wave(lib, ldy=3) < 0
    assert _wave(lib, work=FAKE + 4) < 0 and b"8-byte aligned" in lib.clskd_last_error()


def _wgrad(lib, s=FAKE, y=FAKE, B=2, L=100, coef=FAKE, d=FAKE, ldd=100):
    return lib.clskd_wave_loss_grad(s, 100, y, 100, B, L, coef, d, ldd, 0, None)


def test_wave_loss_grad_rejects_bad_arguments():
    lib = _lib.load(require_gpu=False)
    assert _wgrad(lib, s=None) == -4 and b"wave_loss_grad: null pointer" in lib.clskd_last_error()
    assert _wgrad(lib, coef=None) == -4
    assert _wgrad(lib, d=None) == -4
    assert _wgrad(lib, B=0) < 0
    assert _wgrad(lib, L=0) < 0
    assert _wgrad(lib, ldd=99) < 0 and b"ldd=99" in lib.clskd_last_error()


def _mel(lib, clean=FAKE, est=FAKE, ldc=514, lde=516, B=2, T=19, tab=FAKE, work=FAKE, out=FAKE):
    return lib.clskd_mel_loss(clean, ldc, est, lde, B, T, tab, work, 1.0, 0, out, None)


def _melb(lib, clean=FAKE, est=FAKE, ldc=514, lde=516, B=2, T=19, tab=FAKE, d=FAKE, ldd=516):
    return lib.clskd_mel_loss_bwd(clean, ldc, est, lde, B, T, tab, 1.0, d, ldd, 0, None)


def test_mel_loss_rejects_bad_arguments():
    lib = _lib.load(require_gpu=False)
    for fn, name in ((_mel, b"mel_loss"), (_melb, b"mel_loss_bwd")):
        assert fn(lib, clean=None) == -4 and name + b": null pointer" in lib.clskd_last_error()
        assert fn(lib, est=None) == -4
        assert fn(lib, tab=None) == -4
        assert fn(lib, B=0) < 0 and b"B=0" in lib.clskd_last_error()
        assert fn(lib, T=0) < 0 and b"T=0" in lib.clskd_last_error()
        assert fn(lib, T=(1 << 22) + 1) < 0
        assert fn(lib, ldc=513) < 0 and b"ldc=513" in lib.clskd_last_error()
        assert fn(lib, lde=512) < 0 and b"lde=512" in lib.clskd_last_error()
    assert _mel(lib, work=None) == -4
    assert _mel(lib, out=None) == -4
    assert _mel(lib, work=FAKE + 4) < 0 and b"8-byte aligned" in lib.clskd_last_error()
    assert _melb(lib, d=None) == -4
    assert _melb(lib, ldd=513) < 0 and b"ldd=513" in lib.clskd_last_error()


def test_workspace_queries_are_monotone_and_bounded():
    lib = _lib.load(require_gpu=False)
    assert lib.clskd_wave_loss_workspace(0, 100) == 0 and lib.clskd_wave_loss_workspace(2, 0) == 0
    assert lib.clskd_mel_loss_workspace(0, 19) == 0 and lib.clskd_mel_loss_workspace(2, 0) == 0
    prev = 0
    for L in (1, 7, 1600, 4096, 4097, 48000, 70001, 10 ** 6, 2 ** 31 - 1):
        w = lib.clskd_wave_loss_workspace(3, L)
        assert prev <= w <= 3 * (64 * 4 + 4), (L, w)  # at most 64 blocks of 4 partials per row
        prev = w
    assert lib.clskd_wave_loss_workspace(1, 1) == 8
    assert lib.clskd_wave_loss_workspace(32, 48000) == 32 * (12 * 4 + 4)
    prev = 0
    for B in (1, 2, 32, 65535):
        w = lib.clskd_wave_loss_workspace(B, 48000)
        assert prev < w
        prev = w
    prev = 0
    for T in (1, 2, 19, 32, 33, 163, 257, 300, 481, 1 << 22):
        w = lib.clskd_mel_loss_workspace(3, T)
        assert prev <= w == 3 * ((T + 31) // 32), (T, w)
        prev = w
