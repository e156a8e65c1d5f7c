"""CPU: the entries of csrc/mini_bwd.hip validate their arguments before any launch — null
pointers, a channel count that is not a multiple of 4 and bad extents come back as a status code
with a clskd_last_error text (no GPU compute is called)."""
from clskd import _lib

FAKE = 1 << 20  # never dereferenced: validation fails first


def test_mask_bdt_bwd_rejects_bad_arguments():
    lib = _lib.load(require_gpu=False)
    assert lib.clskd_mask_bdt_bwd(None, 514, FAKE, 5, 2, 5, FAKE, 516, FAKE, None) == -4
    assert b"mask_bdt_bwd: null pointer" in lib.clskd_last_error()
    assert lib.clskd_mask_bdt_bwd(FAKE, 514, FAKE, 5, 2, 5, FAKE, 516, None, None) == -4
    assert lib.clskd_mask_bdt_bwd(FAKE, 514, FAKE, 4, 2, 5, FAKE, 516, FAKE, None) < 0
    assert b"Tm=4" in lib.clskd_last_error()
    assert lib.clskd_mask_bdt_bwd(FAKE, 514, FAKE, 5, 0, 5, FAKE, 516, FAKE, None) < 0
    assert lib.clskd_mask_bdt_bwd(FAKE, 514, FAKE, 5, 2, 5, FAKE, 512, FAKE, None) < 0
    assert b"ldest=512" in lib.clskd_last_error()


def _bn(lib, x=FAKE, C=8, work=FAKE, alpha=FAKE, dx=FAKE, rows=16):
    return lib.clskd_bn_bwd_reim(x, FAKE, rows, C, FAKE, FAKE, FAKE, FAKE, 1e-5, FAKE, alpha, work,
                                 1, None, None, None, dx, 0, 0, None)


def test_bn_bwd_reim_rejects_bad_arguments():
    lib = _lib.load(require_gpu=False)
    assert _bn(lib, x=None) == -4 and b"bn_bwd_reim: null pointer" in lib.clskd_last_error()
    assert _bn(lib, alpha=None) == -4
    assert _bn(lib, dx=None) == -4
    for C in (7, 6, 2, 0, 1028):  # odd, even but not a multiple of 4, too small, too wide
        assert _bn(lib, C=C) < 0, C
        assert f"C={C}".encode() in lib.clskd_last_error()
    assert _bn(lib, rows=0) < 0
    assert _bn(lib, work=FAKE + 8) < 0 and b"16-byte aligned" in lib.clskd_last_error()


def test_mse_loss_grad_rejects_bad_arguments():
    lib = _lib.load(require_gpu=False)
    assert lib.clskd_mse_loss_grad(None, FAKE, 8, 1.0, FAKE, FAKE, None, 0, None) == -4
    assert b"mse_loss_grad: null pointer" in lib.clskd_last_error()
    assert lib.clskd_mse_loss_grad(FAKE, FAKE, 8, 1.0, None, FAKE, None, 0, None) == -4
    assert lib.clskd_mse_loss_grad(FAKE, FAKE, 8, 1.0, FAKE, None, None, 0, None) == -4
    assert lib.clskd_mse_loss_grad(FAKE, FAKE, 0, 1.0, FAKE, FAKE, None, 0, None) < 0
    assert b"n=0" in lib.clskd_last_error()
    assert lib.clskd_mse_loss_grad_workspace(1) == 1
    assert 1 <= lib.clskd_mse_loss_grad_workspace(32 * 48000) <= 1024
