"""CPU: clskd_mask_cr / clskd_mask_cr_bwd validate their arguments before any launch — null
pointers, a mask shorter than T + 1 frames, an empty batch, a row pitch under 514 and an unknown
mode come back as a status code with a clskd_last_error text (no GPU compute is called)."""
import pytest

from clskd import _lib

FAKE = 1 << 20  # never dereferenced: validation fails first
C, R = 1, 2     # CLSKD_MASK_C, CLSKD_MASK_R


def _fwd(lib, mode=C, spec=FAKE, ldspec=514, mask=FAKE, Tm=6, B=2, T=5, est=FAKE, ldest=516,
         mr=None, mi=None):
    return lib.clskd_mask_cr(mode, spec, ldspec, mask, Tm, B, T, est, ldest, mr, mi, None)


def _bwd(lib, mode=C, spec=FAKE, ldspec=514, mask=FAKE, Tm=6, B=2, T=5, dest=FAKE, ldest=516,
         dmask=FAKE):
    return lib.clskd_mask_cr_bwd(mode, spec, ldspec, mask, Tm, B, T, dest, ldest, dmask, None)


@pytest.mark.parametrize("mode", [C, R])
def test_mask_cr_rejects_bad_arguments(mode):
    lib = _lib.load(require_gpu=False)
    for kw in (dict(spec=None), dict(mask=None), dict(est=None)):
        assert _fwd(lib, mode, **kw) == -4, kw
        assert b"mask_cr: null pointer" in lib.clskd_last_error()
    assert _fwd(lib, mode, mr=FAKE) == -4  # mask_r without mask_i
    assert _fwd(lib, mode, Tm=5) < 0 and b"Tm=5" in lib.clskd_last_error()
    assert _fwd(lib, mode, B=0) < 0 and b"B=0" in lib.clskd_last_error()
    assert _fwd(lib, mode, T=0, Tm=1) < 0
    assert _fwd(lib, mode, ldest=512) < 0 and b"ldest=512" in lib.clskd_last_error()
    assert _fwd(lib, mode, ldest=772) < 0  # more tail columns than one pass over 257 bins zeroes
    assert _fwd(lib, mode, ldspec=513) < 0 and b"ldspec=513" in lib.clskd_last_error()


@pytest.mark.parametrize("mode", [C, R])
def test_mask_cr_bwd_rejects_bad_arguments(mode):
    lib = _lib.load(require_gpu=False)
    for kw in (dict(spec=None), dict(mask=None), dict(dest=None), dict(dmask=None)):
        assert _bwd(lib, mode, **kw) == -4, kw
        assert b"mask_cr_bwd: null pointer" in lib.clskd_last_error()
    assert _bwd(lib, mode, Tm=5) < 0 and b"Tm=5" in lib.clskd_last_error()
    assert _bwd(lib, mode, B=0) < 0 and b"B=0" in lib.clskd_last_error()
    assert _bwd(lib, mode, ldest=512) < 0 and b"ldest=512" in lib.clskd_last_error()
    assert _bwd(lib, mode, ldspec=100) < 0


def test_unknown_mode_is_refused():
    lib = _lib.load(require_gpu=False)
    for mode in (0, 3, -1, ord("C")):
        assert _fwd(lib, mode) < 0 and f"mode={mode}".encode() in lib.clskd_last_error()
        assert _bwd(lib, mode) < 0 and f"mode={mode}".encode() in lib.clskd_last_error()
