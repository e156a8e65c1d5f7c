"""Shapes shared by the halo-tiled split-product conv tests (csrc/conv_halo_split.hip): the plan
check on the host (test_halo_split_plan.py) and the GPU parity tests (test_gpu_halo_split.py)."""

ENC = [(kf - 2, kt - 1) for kf in range(5) for kt in range(2)]
DEC0 = [(dF, -kt) for dF in (1, 0, -1) for kt in (0, 1)]
DEC1 = [(dF, -kt) for dF in (1, 0) for kt in (0, 1)]
ABF = [(kf - 1, kt - 1) for kf in range(3) for kt in range(3)]

T = 101  # three full 32-step T tiles and a ragged one of 5

# name: (B, segment channels, N, taps, stride_f, Fi, Fo, of_mul, of_add, column halves)
# B = 3 gives 36 tiles of 8 x 32 for Fo 17..20; the 4-row layer (tiles of 4 x 64, two per batch
# element at T = 101) takes B = 16 to reach the 32 tiles below which the kernel leaves a layer to
# conv_split3_kernel.
CASES = {
    "enc_n64": (3, (32,), 64, ENC, 2, 40, 20, 1, 0, 1),
    "enc_n32": (3, (16,), 32, ENC, 2, 33, 17, 1, 0, 1),
    "enc_fo4_n64_k640": (16, (64,), 64, ENC, 2, 8, 4, 1, 0, 2),
    "dec_p0_n64_k768": (3, (64, 64), 64, DEC0, 1, 20, 20, 2, 0, 2),
    "dec_p1_n32": (3, (32, 32), 32, DEC1, 1, 20, 20, 2, 1, 1),
    "enc_n48": (3, (16,), 48, ENC, 2, 40, 20, 1, 0, 1),
    "enc_n16": (3, (16,), 16, ENC, 2, 40, 20, 1, 0, 1),
    "abf3x3_n64": (3, (8,), 64, ABF, 1, 20, 20, 1, 0, 1),
}

# the student's split-product MFMA launches of the benchmarked step (B = 16, T = 643)
STUDENT = {
    "enc2": (16, (16,), 32, ENC, 2, 64, 32, 1, 0),
    "enc3": (16, (32,), 64, ENC, 2, 32, 16, 1, 0),
    "enc4": (16, (64,), 64, ENC, 2, 16, 8, 1, 0),
    "enc5": (16, (64,), 64, ENC, 2, 8, 4, 1, 0),
    "dec0p0": (16, (64, 64), 64, DEC0, 1, 4, 4, 2, 0),
    "dec0p1": (16, (64, 64), 64, DEC1, 1, 4, 4, 2, 1),
    "dec1p0": (16, (64, 64), 64, DEC0, 1, 8, 8, 2, 0),
    "dec1p1": (16, (64, 64), 64, DEC1, 1, 8, 8, 2, 1),
    "dec2p0": (16, (64, 64), 32, DEC0, 1, 16, 16, 2, 0),
    "dec2p1": (16, (64, 64), 32, DEC1, 1, 16, 16, 2, 1),
    "dec3p0": (16, (32, 32), 16, DEC0, 1, 32, 32, 2, 0),
    "dec3p1": (16, (32, 32), 16, DEC1, 1, 32, 32, 2, 1),
}
STUDENT_T = 643
