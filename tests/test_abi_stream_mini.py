"""CPU-side checks of the fused DCCRNet_mini hop's C ABI (clskd_stream_hop_mini, include/clskd.h):
the ctypes mirror has the C compiler's layout of clskd_stream_hop_mini_args, and the entry point
validates its arguments before anything is launched.  No GPU is needed."""
import ctypes
import os
import subprocess

from clskd import _lib


def test_mini_args_layout_matches_header(tmp_path):
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    probe = tmp_path / "probe.c"
    probe.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "clskd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\\n", sizeof(clskd_stream_hop_mini_args),
         offsetof(clskd_stream_hop_mini_args, wav_out), offsetof(clskd_stream_hop_mini_args, off_frames),
         offsetof(clskd_stream_hop_mini_args, dec_alpha), offsetof(clskd_stream_hop_mini_args, drain));
  return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", inc, str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    M = _lib.StreamHopMiniArgs
    assert got == [ctypes.sizeof(M), M.wav_out.offset, M.off_frames.offset, M.dec_alpha.offset,
                   M.drain.offset]


def test_mini_hop_validates_before_launch_without_gpu():
    lib = _lib.load(require_gpu=False)
    rc = lib.clskd_stream_hop_mini(None, None)
    assert rc < 0
    assert b"stream_hop_mini" in lib.clskd_last_error()
    # shapes are checked against the LDS budget before anything is launched
    a = _lib.StreamHopMiniArgs()
    fake = 1 << 20  # never dereferenced: validation fails first
    a.state = a.wav_out = a.x_in = a.stft_w = a.istft_w = a.lin_w = a.lin_b = fake
    a.B, a.t, a.live, a.drain, a.H, a.D4 = 1, 0, 1, 0, 64, 4
    for i in range(6):
        a.enc_cout[i] = 64
    assert lib.clskd_stream_hop_mini(ctypes.byref(a), None) < 0
    assert b"LDS budget" in lib.clskd_last_error()
    a.H, a.drain = 32, 2  # a live hop cannot also be a drain hop
    assert lib.clskd_stream_hop_mini(ctypes.byref(a), None) < 0
    assert b"drain" in lib.clskd_last_error()
