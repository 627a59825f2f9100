"""Case tables, input families, references and comparisons for the reduction kernels (tests/test_gpu_reductions.py on the
device, tests/test_host_reduction_cases.py without one): the column sums of csrc/colsum.hip, the per-block partial rows of the
LayerNorm and GroupNorm backwards, the Huber loss, the clip norm with the AdamW update, and the parameter checksum.

Two input families.  EXACT: integer-valued fp32 in [-8, 8] -- every partial sum in any order is an integer below 2^24, so the
device result must EQUAL the int64 sum cast to fp32 (torch.equal, no tolerance); dropout p = 0.5 (multiplier 2), the scales
1, 0.25, -2 and an integer-valued `out` to accumulate onto keep it exact.  A row, column, segment or partial row that is
dropped, doubled or misaddressed changes an integer.  REAL: N(0, 1) against float64 with the forward error bound that holds
for any summation order, |got - ref| <= gamma_n * sum|addend_i| + one fp32 ulp of ref, gamma_n = n u / (1 - n u), u = 2^-24,
n the number of addends (`out` is one when accumulating; the scales are powers of two and the p = 0.5 multiplier is exact,
so the n - 1 additions and the one multiplication by the scale are the only roundings).  It is loose by design: it catches
a wrong scale, rounding or mask; the exact family catches omissions.

Nothing here needs a GPU: every function takes tensors on whatever device they live on."""
import math
import zlib
from typing import NamedTuple

import numpy as np
import torch

U = 2.0 ** -24
SENTINEL = -12345.0                  # what the surroundings of every output window hold before a launch
MASK_SEED = 0x5EED5EED12345
NAN = float("nan")


def gen(*key):
    """A CPU generator seeded by the case, so that every test and the host self-check see the same values."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def gamma_n(n):
    return n * U / (1.0 - n * U)


def ulp32(ref64):
    """One fp32 unit in the last place of every element of a float64 tensor."""
    r = ref64.float().abs()
    return (torch.nextafter(r, torch.full_like(r, float("inf"))) - r).double()


def need_dev(got, ref, row_dims):
    """tests/hard_inputs.py: need(), evaluated where the tensors live (no copy of an (M, D) float64 tensor to the host):
    the smallest t with |got - ref| <= t * (|ref| + 0.1 rms_row(ref) + 0.01 rms_all(ref)); inf for a non-finite element."""
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rms_all = ref.pow(2).mean().sqrt()
    rms_row = ref.abs() if row_dims == () else (rms_all if row_dims is None else ref.pow(2).mean(dim=row_dims, keepdim=True).sqrt())
    den = ref.abs() + 0.1 * rms_row + 0.01 * rms_all
    d = (got - ref).abs()
    t = torch.where(d == 0, torch.zeros_like(d), d / den)
    t = torch.where(torch.isfinite(got), t, torch.full_like(t, float("inf")))
    return float(t.max())


# ================================================================================================ column sums
class Colsum(NamedTuple):
    name: str
    C: int
    ld: int
    off: int            # floats between a 16-byte boundary and the first element of the input
    outer: int
    inner: int
    nseg: int
    p: float            # dropout on the input (0: no mask); the mask index is row * drop_ld + column
    drop_ld: int
    scale: float
    acc: int
    route: str          # what tecm_colsum_path answers

    @property
    def total(self):    # rows per segment
        return self.outer * self.inner

    @property
    def rows(self):
        return self.outer * self.inner * self.nseg

    @property
    def stage1(self):
        return self.route.split()[0]

    @property
    def rb(self):
        return int(self.route.split("rb=")[1].split()[0])

    @property
    def chunk(self):
        return int(self.route.split("chunk=")[1].split()[0])

    @property
    def waves(self):
        return int(self.route.split("waves=")[1].split()[0])

    @property
    def colblocks(self):
        return (self.C + 63) // 64


# One axis at a time off the ragged base case (C = 68, 37 x 5 rows in each of 3 segments, ld = C, aligned); wide C with few
# rows, many rows with narrow C (the largest input, 70000 x 64, is 18 MB).  The options (p, scale, accumulate) cycle through
# (0, 1, 0), (0.5, 0.25, 1), (0, -2, 0), (0.5, 1, 0), (0, 0.25, 1), (0.5, -2, 1) down the table; inputs of more than 2^21
# elements carry no mask (the mask is mirrored on the host).
_COLSUM = [
    # --- C, either side of the quad, of one and four 64-column blocks and of the float4 stage's 1024-column limit
    ("C1", 1, 1, 0, 37, 5, 3, 0.0, 1, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("C3", 3, 3, 0, 37, 5, 3, 0.5, 3, 0.25, 1, "scalar rb=12 chunk=16 waves=8"),
    ("C4", 4, 4, 0, 37, 5, 3, 0.0, 4, -2.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("C60", 60, 60, 0, 37, 5, 3, 0.5, 60, 1.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("C64", 64, 64, 0, 37, 5, 3, 0.0, 64, 0.25, 1, "v4 rb=12 chunk=16 waves=8"),
    ("C68", 68, 68, 0, 37, 5, 3, 0.5, 68, -2.0, 1, "v4 rb=12 chunk=16 waves=8"),
    ("C252", 252, 252, 0, 37, 5, 3, 0.0, 252, 1.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("C256", 256, 256, 0, 37, 5, 3, 0.5, 256, 0.25, 1, "v4 rb=12 chunk=16 waves=8"),
    ("C260", 260, 260, 0, 37, 5, 3, 0.0, 260, -2.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("C1020", 1020, 1020, 0, 37, 5, 3, 0.5, 1020, 1.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("C1024", 1024, 1024, 0, 37, 5, 3, 0.0, 1024, 0.25, 1, "v4 rb=12 chunk=16 waves=8"),
    ("C1028", 1028, 1028, 0, 37, 5, 3, 0.5, 1028, -2.0, 1, "scalar rb=12 chunk=16 waves=8"),
    ("C1536", 1536, 1536, 0, 37, 5, 3, 0.0, 1536, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("C2304", 2304, 2304, 0, 37, 5, 3, 0.5, 2304, 0.25, 1, "scalar rb=9 chunk=21 waves=8"),
    # --- ld in {C, C + 4, C + 1}
    ("C68_ld+0", 68, 68, 0, 37, 5, 3, 0.0, 68, -2.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("C68_ld+4", 68, 72, 0, 37, 5, 3, 0.5, 72, 1.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("C68_ld+1", 68, 69, 0, 37, 5, 3, 0.0, 69, 0.25, 1, "scalar rb=12 chunk=16 waves=8"),
    ("C70_ld+0", 70, 70, 0, 37, 5, 3, 0.5, 70, -2.0, 1, "scalar rb=12 chunk=16 waves=8"),
    ("C70_ld+4", 70, 74, 0, 37, 5, 3, 0.0, 74, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("C70_ld+1", 70, 71, 0, 37, 5, 3, 0.5, 71, 0.25, 1, "scalar rb=12 chunk=16 waves=8"),
    ("C1028_ld+0", 1028, 1028, 0, 37, 5, 3, 0.0, 1028, -2.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("C1028_ld+4", 1028, 1032, 0, 37, 5, 3, 0.5, 1032, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("C1028_ld+1", 1028, 1029, 0, 37, 5, 3, 0.0, 1029, 0.25, 1, "scalar rb=12 chunk=16 waves=8"),
    # --- the input 0, 1 and 4 floats past a 16-byte boundary
    ("C68_off0", 68, 68, 0, 37, 5, 3, 0.5, 68, -2.0, 1, "v4 rb=12 chunk=16 waves=8"),
    ("C68_off1", 68, 68, 1, 37, 5, 3, 0.0, 68, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("C68_off4", 68, 68, 4, 37, 5, 3, 0.5, 68, 0.25, 1, "v4 rb=12 chunk=16 waves=8"),
    ("C70_off0", 70, 70, 0, 37, 5, 3, 0.0, 70, -2.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("C70_off1", 70, 70, 1, 37, 5, 3, 0.5, 70, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("C70_off4", 70, 70, 4, 37, 5, 3, 0.0, 70, 0.25, 1, "scalar rb=12 chunk=16 waves=8"),
    # --- total rows: the 16-rows-per-block clamp, 256 and 1024 partial rows, the 1024 / nseg clamp with a ragged last chunk
    ("rows1_C64", 64, 64, 0, 1, 1, 1, 0.5, 64, -2.0, 1, "v4 rb=1 chunk=1 waves=8"),
    ("rows15_C64", 64, 64, 0, 15, 1, 1, 0.0, 64, 1.0, 0, "v4 rb=1 chunk=15 waves=8"),
    ("rows16_C64", 64, 64, 0, 16, 1, 1, 0.5, 64, 0.25, 1, "v4 rb=1 chunk=16 waves=8"),
    ("rows17_C64", 64, 64, 0, 17, 1, 1, 0.0, 64, -2.0, 0, "v4 rb=2 chunk=9 waves=8"),
    ("rows4095_C64", 64, 64, 0, 4095, 1, 1, 0.5, 64, 1.0, 0, "v4 rb=256 chunk=16 waves=8"),
    ("rows4096_C64", 64, 64, 0, 4096, 1, 1, 0.0, 64, 0.25, 1, "v4 rb=256 chunk=16 waves=8"),
    ("rows4097_C64", 64, 64, 0, 4097, 1, 1, 0.5, 64, -2.0, 1, "v4 rb=257 chunk=16 waves=16"),
    ("rows16383_C64", 64, 64, 0, 16383, 1, 1, 0.0, 64, 1.0, 0, "v4 rb=1024 chunk=16 waves=16"),
    ("rows16384_C64", 64, 64, 0, 16384, 1, 1, 0.5, 64, 0.25, 1, "v4 rb=1024 chunk=16 waves=16"),
    ("rows16385_C64", 64, 64, 0, 16385, 1, 1, 0.0, 64, -2.0, 0, "v4 rb=964 chunk=17 waves=16"),
    ("rows20000_C64", 64, 64, 0, 20000, 1, 1, 0.5, 64, 1.0, 0, "v4 rb=1000 chunk=20 waves=16"),
    ("rows70000_C64", 64, 64, 0, 70000, 1, 1, 0.0, 64, 0.25, 1, "v4 rb=1015 chunk=69 waves=16"),
    ("rows1_C3", 3, 3, 0, 1, 1, 1, 0.5, 3, -2.0, 1, "scalar rb=1 chunk=1 waves=8"),
    ("rows15_C3", 3, 3, 0, 15, 1, 1, 0.0, 3, 1.0, 0, "scalar rb=1 chunk=15 waves=8"),
    ("rows16_C3", 3, 3, 0, 16, 1, 1, 0.5, 3, 0.25, 1, "scalar rb=1 chunk=16 waves=8"),
    ("rows17_C3", 3, 3, 0, 17, 1, 1, 0.0, 3, -2.0, 0, "scalar rb=2 chunk=9 waves=8"),
    ("rows4095_C3", 3, 3, 0, 4095, 1, 1, 0.5, 3, 1.0, 0, "scalar rb=256 chunk=16 waves=8"),
    ("rows4096_C3", 3, 3, 0, 4096, 1, 1, 0.0, 3, 0.25, 1, "scalar rb=256 chunk=16 waves=8"),
    ("rows4097_C3", 3, 3, 0, 4097, 1, 1, 0.5, 3, -2.0, 1, "scalar rb=241 chunk=17 waves=8"),
    ("rows16383_C3", 3, 3, 0, 16383, 1, 1, 0.0, 3, 1.0, 0, "scalar rb=256 chunk=64 waves=8"),
    ("rows16384_C3", 3, 3, 0, 16384, 1, 1, 0.5, 3, 0.25, 1, "scalar rb=256 chunk=64 waves=8"),
    ("rows16385_C3", 3, 3, 0, 16385, 1, 1, 0.0, 3, -2.0, 0, "scalar rb=253 chunk=65 waves=8"),
    ("rows20000_C3", 3, 3, 0, 20000, 1, 1, 0.5, 3, 1.0, 0, "scalar rb=254 chunk=79 waves=8"),
    ("rows70000_C3", 3, 3, 0, 70000, 1, 1, 0.0, 3, 0.25, 1, "scalar rb=256 chunk=274 waves=8"),
    ("rows1_C1028", 1028, 1028, 0, 1, 1, 1, 0.5, 1028, -2.0, 1, "scalar rb=1 chunk=1 waves=8"),
    ("rows15_C1028", 1028, 1028, 0, 15, 1, 1, 0.0, 1028, 1.0, 0, "scalar rb=1 chunk=15 waves=8"),
    ("rows16_C1028", 1028, 1028, 0, 16, 1, 1, 0.5, 1028, 0.25, 1, "scalar rb=1 chunk=16 waves=8"),
    ("rows17_C1028", 1028, 1028, 0, 17, 1, 1, 0.0, 1028, -2.0, 0, "scalar rb=2 chunk=9 waves=8"),
    ("rows4095_C1028", 1028, 1028, 0, 4095, 1, 1, 0.0, 1028, 1.0, 0, "scalar rb=60 chunk=69 waves=8"),
    ("rows4096_C1028", 1028, 1028, 0, 4096, 1, 1, 0.0, 1028, 0.25, 1, "scalar rb=60 chunk=69 waves=8"),
    ("rows4097_C1028", 1028, 1028, 0, 4097, 1, 1, 0.0, 1028, -2.0, 1, "scalar rb=60 chunk=69 waves=8"),
    # --- nseg in {1, 3, 4, 5} x inner in {1, 5, 211}, on both first stages
    ("C68_nseg1_inner1", 68, 68, 0, 7, 1, 1, 0.0, 68, 1.0, 0, "v4 rb=1 chunk=7 waves=8"),
    ("C68_nseg1_inner5", 68, 68, 0, 7, 5, 1, 0.5, 68, 0.25, 1, "v4 rb=3 chunk=12 waves=8"),
    ("C68_nseg1_inner211", 68, 68, 0, 7, 211, 1, 0.0, 68, -2.0, 0, "v4 rb=93 chunk=16 waves=8"),
    ("C68_nseg3_inner1", 68, 68, 0, 7, 1, 3, 0.5, 68, 1.0, 0, "v4 rb=1 chunk=7 waves=8"),
    ("C68_nseg3_inner5", 68, 68, 0, 7, 5, 3, 0.0, 68, 0.25, 1, "v4 rb=3 chunk=12 waves=8"),
    ("C68_nseg3_inner211", 68, 68, 0, 7, 211, 3, 0.5, 68, -2.0, 1, "v4 rb=93 chunk=16 waves=8"),
    ("C68_nseg4_inner1", 68, 68, 0, 7, 1, 4, 0.0, 68, 1.0, 0, "v4 rb=1 chunk=7 waves=8"),
    ("C68_nseg4_inner5", 68, 68, 0, 7, 5, 4, 0.5, 68, 0.25, 1, "v4 rb=3 chunk=12 waves=8"),
    ("C68_nseg4_inner211", 68, 68, 0, 7, 211, 4, 0.0, 68, -2.0, 0, "v4 rb=93 chunk=16 waves=8"),
    ("C68_nseg5_inner1", 68, 68, 0, 7, 1, 5, 0.5, 68, 1.0, 0, "v4 rb=1 chunk=7 waves=8"),
    ("C68_nseg5_inner5", 68, 68, 0, 7, 5, 5, 0.0, 68, 0.25, 1, "v4 rb=3 chunk=12 waves=8"),
    ("C68_nseg5_inner211", 68, 68, 0, 7, 211, 5, 0.5, 68, -2.0, 1, "v4 rb=93 chunk=16 waves=8"),
    ("C70_nseg1_inner1", 70, 70, 0, 7, 1, 1, 0.0, 70, 1.0, 0, "scalar rb=1 chunk=7 waves=8"),
    ("C70_nseg1_inner5", 70, 70, 0, 7, 5, 1, 0.5, 70, 0.25, 1, "scalar rb=3 chunk=12 waves=8"),
    ("C70_nseg1_inner211", 70, 70, 0, 7, 211, 1, 0.0, 70, -2.0, 0, "scalar rb=93 chunk=16 waves=8"),
    ("C70_nseg3_inner1", 70, 70, 0, 7, 1, 3, 0.5, 70, 1.0, 0, "scalar rb=1 chunk=7 waves=8"),
    ("C70_nseg3_inner5", 70, 70, 0, 7, 5, 3, 0.0, 70, 0.25, 1, "scalar rb=3 chunk=12 waves=8"),
    ("C70_nseg3_inner211", 70, 70, 0, 7, 211, 3, 0.5, 70, -2.0, 1, "scalar rb=93 chunk=16 waves=8"),
    ("C70_nseg4_inner1", 70, 70, 0, 7, 1, 4, 0.0, 70, 1.0, 0, "scalar rb=1 chunk=7 waves=8"),
    ("C70_nseg4_inner5", 70, 70, 0, 7, 5, 4, 0.5, 70, 0.25, 1, "scalar rb=3 chunk=12 waves=8"),
    ("C70_nseg4_inner211", 70, 70, 0, 7, 211, 4, 0.0, 70, -2.0, 0, "scalar rb=93 chunk=16 waves=8"),
    ("C70_nseg5_inner1", 70, 70, 0, 7, 1, 5, 0.5, 70, 1.0, 0, "scalar rb=1 chunk=7 waves=8"),
    ("C70_nseg5_inner5", 70, 70, 0, 7, 5, 5, 0.0, 70, 0.25, 1, "scalar rb=3 chunk=12 waves=8"),
    ("C70_nseg5_inner211", 70, 70, 0, 7, 211, 5, 0.5, 70, -2.0, 1, "scalar rb=93 chunk=16 waves=8"),
    # --- partial rows either side of 256 with colblocks * nseg either side of 4: the 16-wave second stage and its neighbours
    ("parts_C256_nseg1_rows4096", 256, 256, 0, 4096, 1, 1, 0.0, 256, 1.0, 0, "v4 rb=256 chunk=16 waves=8"),
    ("parts_C256_nseg1_rows4097", 256, 256, 0, 4097, 1, 1, 0.5, 256, 0.25, 1, "v4 rb=257 chunk=16 waves=16"),
    ("parts_C260_nseg1_rows4097", 260, 260, 0, 4097, 1, 1, 0.0, 260, -2.0, 0, "v4 rb=257 chunk=16 waves=8"),
    ("parts_C252_nseg1_rows4097", 252, 252, 0, 4097, 1, 1, 0.5, 252, 1.0, 0, "v4 rb=257 chunk=16 waves=16"),
    ("parts_C64_nseg3_rows4096", 64, 64, 0, 4096, 1, 3, 0.0, 64, 0.25, 1, "v4 rb=256 chunk=16 waves=8"),
    ("parts_C64_nseg3_rows4097", 64, 64, 0, 4097, 1, 3, 0.5, 64, -2.0, 1, "v4 rb=257 chunk=16 waves=16"),
    ("parts_C128_nseg2_rows4097", 128, 128, 0, 4097, 1, 2, 0.0, 128, 1.0, 0, "v4 rb=257 chunk=16 waves=16"),
    ("parts_C192_nseg2_rows4097", 192, 192, 0, 4097, 1, 2, 0.5, 192, 0.25, 1, "v4 rb=257 chunk=16 waves=8"),
    ("parts_C64_nseg4_rows4097", 64, 64, 0, 4097, 1, 4, 0.0, 64, -2.0, 0, "v4 rb=241 chunk=17 waves=8"),
    ("parts_C64_nseg5_rows4097", 64, 64, 0, 4097, 1, 5, 0.5, 64, 1.0, 0, "v4 rb=196 chunk=21 waves=8"),
    ("parts_C70_nseg2_rows4096", 70, 70, 0, 4096, 1, 2, 0.0, 70, 0.25, 1, "scalar rb=256 chunk=16 waves=8"),
    ("parts_C70_nseg2_rows4097", 70, 70, 0, 4097, 1, 2, 0.5, 70, -2.0, 1, "scalar rb=241 chunk=17 waves=8"),
    ("parts_C70_nseg4_rows4097", 70, 70, 0, 4097, 1, 4, 0.0, 70, 1.0, 0, "scalar rb=125 chunk=33 waves=8"),
    ("parts_C3_nseg5_rows4097", 3, 3, 0, 4097, 1, 5, 0.5, 3, 0.25, 1, "scalar rb=196 chunk=21 waves=8"),
    ("parts_C64_nseg1_rows16400", 64, 64, 0, 16400, 1, 1, 0.0, 64, -2.0, 0, "v4 rb=965 chunk=17 waves=16"),
    # --- masks on and off, with a mask index built on another leading dimension than the input's
    ("mask_C68_ld72_dropld72", 68, 72, 0, 37, 5, 3, 0.5, 72, 1.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("mask_C68_ld72_dropld75", 68, 72, 0, 37, 5, 3, 0.5, 75, 1.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("mask_C68_ld72_dropld68", 68, 72, 0, 37, 5, 3, 0.5, 68, 1.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("nomask_C68_ld72", 68, 72, 0, 37, 5, 3, 0.0, 72, 1.0, 0, "v4 rb=12 chunk=16 waves=8"),
    ("mask_C70_ld70_dropld70", 70, 70, 0, 37, 5, 3, 0.5, 70, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("mask_C70_ld70_dropld73", 70, 70, 0, 37, 5, 3, 0.5, 73, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("mask_C70_ld70_dropld78", 70, 70, 0, 37, 5, 3, 0.5, 78, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
    ("nomask_C70_ld70", 70, 70, 0, 37, 5, 3, 0.0, 70, 1.0, 0, "scalar rb=12 chunk=16 waves=8"),
]
COLSUM = [Colsum(*row) for row in _COLSUM]

# The second stage runs 16 waves only behind more than 256 partial rows, and the lane-per-column first stages (scalar, batch)
# never leave more than 256 (their block count is clamped to 256): (first stage, waves) pairs the launchers can reach.  The
# host test proves the other two unreachable over a sweep of the query.
COLSUM_ROUTES = {("scalar", 8), ("v4", 8), ("v4", 16), ("batch", 8), ("each", 8), ("each", 16)}
COLSUM_UNREACHABLE = {("scalar", 16), ("batch", 16)}

# The edges every table must hit on BOTH sides: name -> predicate of a case.
COLSUM_EDGES = {
    "C % 4": lambda c: c.C % 4 == 0,
    "C <= 1024": lambda c: c.C <= 1024,
    "ld % 4 (C % 4 == 0, C <= 1024)": lambda c: c.ld % 4 == 0 if (c.C % 4 == 0 and c.C <= 1024) else None,
    "input aligned (C % 4 == 0, ld % 4 == 0)": lambda c: c.off % 4 == 0 if (c.C % 4 == 0 and c.ld % 4 == 0 and c.C <= 1024) else None,
    "ld > C": lambda c: c.ld > c.C,
    "colblocks * nseg <= 4 (rb > 256)": lambda c: c.colblocks * c.nseg <= 4 if c.rb > 256 else None,
    "rb > 256 (colblocks * nseg <= 4)": lambda c: c.rb > 256 if c.colblocks * c.nseg <= 4 else None,
    "v4 block count at the 1024 / nseg clamp": lambda c: (c.total + 15) // 16 >= 1024 // c.nseg if c.stage1 == "v4" else None,
    "ragged last chunk": lambda c: c.total % c.chunk != 0,
    "fewer than 16 rows": lambda c: c.total < 16,
    "scalar block count at its 256 clamp": lambda c: c.rb == 256 if c.stage1 == "scalar" else None,
    "nseg > 1": lambda c: c.nseg > 1,
    "inner > 1": lambda c: c.inner > 1,
    "masked": lambda c: c.p > 0,
    "mask index on the input's ld": lambda c: c.drop_ld == c.ld if c.p > 0 else None,
    "accumulate": lambda c: bool(c.acc),
    "scale != 1": lambda c: c.scale != 1.0,
    "total % 4 (rows in flight)": lambda c: c.total % 4 == 0,
}


def colsum_buffer(c, family):
    """The flat fp32 buffer a case reads: `off` floats, then rows x ld with the values in the first C columns.  Padding columns
    and the floats around the matrix are NaN: a kernel that reads one of them into a sum shows it."""
    g = gen("colsum", c.name, family)
    vals = (torch.randint(-8, 9, (c.rows, c.C), generator=g).float() if family == "exact"
            else torch.randn(c.rows, c.C, generator=g))
    buf = torch.full((c.off + c.rows * c.ld + 4,), NAN)
    buf[c.off:c.off + c.rows * c.ld].view(c.rows, c.ld)[:, :c.C] = vals
    return buf


def colsum_values(buf, c):
    """(outer, nseg, inner, C) view of the values in a buffer: row (o, s, j) is row (o * nseg + s) * inner + j of the matrix."""
    return buf[c.off:c.off + c.rows * c.ld].view(c.outer, c.nseg, c.inner, c.ld)[..., :c.C]


def colsum_mult(c, rows=None, cols=None, drop_ld=None, p=None):
    """(rows, C) fp32 dropout multipliers of the case from the NumPy mirror of the device hash, or None without a mask."""
    from tecmollm import rng
    p = c.p if p is None else p
    if p == 0:
        return None
    rows, cols, drop_ld = rows or c.rows, cols or c.C, drop_ld or c.drop_ld
    idx = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(drop_ld) + np.arange(cols, dtype=np.uint64)[None, :]
    return torch.from_numpy(rng.keep_mult(MASK_SEED, idx, p))


def colsum_out0(c, family):
    """What the (nseg, C) output window holds before the call: the addend of an accumulating case, NaN otherwise."""
    if not c.acc:
        return torch.full((c.nseg, c.C), NAN)
    g = gen("colsum-out", c.name, family)
    return torch.randint(-8, 9, (c.nseg, c.C), generator=g).float() if family == "exact" else torch.randn(c.nseg, c.C, generator=g)


def colsum_int_sums(vals, mult, c):
    """EXACT family: (nseg, total, C) int64 masked values, rows of a segment in the order the kernels walk them."""
    m = vals.to(torch.int64)
    if mult is not None:
        m = m * mult.to(vals.device).view(c.outer, c.nseg, c.inner, c.C).to(torch.int64)
    return m.permute(1, 0, 2, 3).reshape(c.nseg, c.total, c.C)


def colsum_finish_exact(sums, c, out0):
    """int64 (nseg, C) sums -> the fp32 result: scale and the accumulated `out` keep every value exactly representable."""
    r = sums.double() * c.scale
    if c.acc:
        r = r + out0.to(sums.device).double()
    assert float(r.abs().max()) < 2 ** 24
    return r.float()


def colsum_ref_exact(vals, mult, c, out0):
    return colsum_finish_exact(colsum_int_sums(vals, mult, c).sum(1), c, out0)


def colsum_ref_real(vals, mult, c, out0):
    """(float64 reference, bound): |got - ref| <= gamma_n * sum |addend| + ulp32(ref), n addends (`out` is one)."""
    m = vals.double()
    if mult is not None:
        m = m * mult.to(vals.device).view(c.outer, c.nseg, c.inner, c.C).double()
    ref = m.sum((0, 2)) * c.scale
    mass = m.abs().sum((0, 2)) * abs(c.scale)
    n = c.total
    if c.acc:
        o = out0.to(vals.device).double()
        ref, mass, n = ref + o, mass + o.abs(), n + 1
    return ref, gamma_n(n) * mass + ulp32(ref)


def real_ratio(got, ref, bound):
    """Worst |got - ref| / bound (<= 1 passes); inf for a non-finite result."""
    got = got.double()
    r = torch.where(torch.isfinite(got), (got - ref).abs() / bound, torch.full_like(ref, float("inf")))
    return float(r.max())


# What a bug would make of a correct EXACT result: name -> (applies to the case, altered (nseg, C) int64 sums)
def _drop_rows(m, rows):
    keep = torch.ones(m.shape[1], dtype=torch.bool)
    keep[rows] = False
    return m[:, keep].sum(1)


def colsum_alterations(m, c):
    """m: colsum_int_sums.  Yields (name, altered sums) for every alteration the case can show."""
    s = m.sum(1)
    yield "last row of a chunk missing", _drop_rows(m, [c.chunk - 1])
    if c.nseg > 1:
        t = s.clone()
        t[[0, 1]] = s[[1, 0]]
        yield "two segments swapped", t
    t = s.clone()
    t[:, c.C - 1] = 0
    yield "column C - 1 skipped", t
    yield "one partial row counted twice", s + m[:, :c.chunk].sum(1)
    if c.total & 3:
        yield "tail n & 3 skipped", _drop_rows(m, list(range(c.total - (c.total & 3), c.total)))


ALTERATIONS = ("last row of a chunk missing", "two segments swapped", "column C - 1 skipped", "one partial row counted twice",
               "tail n & 3 skipped")


# ---------------------------------------------------------------------------------------------- the bf16 twin
class Twin(NamedTuple):
    name: str
    C: int
    ld: int
    outer: int
    inner: int
    nseg: int
    p: float
    ld_twin: int


TWINS = [Twin("twin_C68_ld72_wide", 68, 72, 37, 5, 3, 0.5, 76), Twin("twin_C68_tight", 68, 68, 37, 5, 3, 0.0, 68),
         Twin("twin_C4", 4, 4, 333, 1, 1, 0.5, 8), Twin("twin_C1024_wide", 1024, 1024, 37, 1, 1, 0.5, 1028),
         Twin("twin_C64_rows4097", 64, 64, 4097, 1, 1, 0.5, 72), Twin("twin_C252_nseg4", 252, 256, 7, 211, 4, 0.0, 252)]
TWIN_REFUSED = [(70, 70, 72), (1028, 1028, 1028), (68, 69, 68)]        # (C, ld, ld_twin): no float4 first stage, no twin


# ---------------------------------------------------------------------------------------------- tecm_colsum_batch
class Batch(NamedTuple):
    name: str
    nbuf: int
    C: int
    rows: int
    misaligned: tuple   # indices of the matrices that start 4 bytes past a 16-byte boundary; (-1,): every one
    route: str

    def is_misaligned(self, i):
        return self.misaligned == (-1,) or i in self.misaligned

    @property
    def best_misalign(self):
        return 4 if all(self.is_misaligned(i) for i in range(self.nbuf)) else 0


# One axis at a time off (nbuf 7, C 1536, 300 rows); "each ...": every matrix goes through tecm_colsum one by one.
BATCH = [Batch(*row) for row in [
    ("nbuf1", 1, 1536, 300, (), "batch rb=19 chunk=16 waves=8 launches=1"),
    ("nbuf7", 7, 1536, 300, (), "batch rb=19 chunk=16 waves=8 launches=1"),
    ("nbuf32", 32, 1536, 300, (), "batch rb=19 chunk=16 waves=8 launches=1"),
    ("nbuf33", 33, 1536, 300, (), "batch rb=19 chunk=16 waves=8 launches=2"),
    ("C6", 7, 6, 300, (), "batch rb=19 chunk=16 waves=8 launches=1"),
    ("C768", 7, 768, 300, (), "each v4 rb=19 chunk=16 waves=8"),
    ("C1028", 7, 1028, 300, (), "batch rb=19 chunk=16 waves=8 launches=1"),
    ("rows1", 7, 1536, 1, (), "batch rb=1 chunk=1 waves=8 launches=1"),
    ("rows4096", 7, 1536, 4096, (), "batch rb=42 chunk=98 waves=8 launches=1"),
    ("rows5000", 7, 1536, 5000, (), "batch rb=42 chunk=120 waves=8 launches=1"),
    ("C64_rows4097", 7, 64, 4097, (), "each v4 rb=257 chunk=16 waves=16"),
    ("C768_one_misaligned", 7, 768, 300, (3,), "each v4 rb=19 chunk=16 waves=8"),
    ("C768_all_misaligned", 7, 768, 300, (-1,), "batch rb=19 chunk=16 waves=8 launches=1"),
    ("C1536_one_misaligned", 7, 1536, 300, (3,), "batch rb=19 chunk=16 waves=8 launches=1"),
    ("C1028_nbuf33", 33, 1028, 300, (), "batch rb=19 chunk=16 waves=8 launches=2"),
    ("C6_nbuf33_rows5000", 33, 6, 5000, (), "batch rb=250 chunk=20 waves=8 launches=2"),
    ("C768_nbuf33_all_misaligned", 33, 768, 300, (-1,), "batch rb=19 chunk=16 waves=8 launches=2"),
]]
BATCH_EDGES = {
    "nbuf > 32 (two launches)": lambda b: b.nbuf > 32,
    "one by one": lambda b: b.route.startswith("each"),
    "C % 4": lambda b: b.C % 4 == 0,
    "C <= 1024": lambda b: b.C <= 1024,
    "a misaligned matrix": lambda b: bool(b.misaligned),
    "every matrix misaligned": lambda b: b.misaligned == (-1,),
    "one row": lambda b: b.rows == 1,
    "nbuf == 1": lambda b: b.nbuf == 1,
}


def batch_matrices(b, family, device):
    """nbuf contiguous (rows, C) fp32 matrices on `device`, each a view into a buffer of its own, 0 or 1 float past the
    16-byte boundary torch allocates on."""
    out = []
    for i in range(b.nbuf):
        g = gen("batch", b.name, family, i)
        vals = torch.randint(-8, 9, (b.rows, b.C), generator=g).float() if family == "exact" else torch.randn(b.rows, b.C, generator=g)
        off = 1 if b.is_misaligned(i) else 0
        buf = torch.full((off + b.rows * b.C + 4,), NAN, device=device)
        m = buf[off:off + b.rows * b.C].view(b.rows, b.C)
        m.copy_(vals)
        assert (m.data_ptr() % 16 == 4) == bool(off)
        out.append(m)
    return out


# ================================================================================================ LayerNorm partials
# ln_blocks: 4 rows a block, 1024 blocks at most: one block, the last block short, the cap, one and many rows past it
LN_M = (1, 3, 4, 5, 4095, 4096, 4097, 8193)
LN_D = (4, 252, 256, 260, 764, 768, 772, 1020, 1024)
LN_REFUSED_D = (1028, 766, 6)
LN_VARIANTS = ("add32", "dy16", "seq_major")         # at D = 768, M = 4097 = 1 x 17 x 241
LN_VARIANT_SHAPE = (4097, 768, (1, 17, 241))


def ln_case_inputs(M, D, device="cpu"):
    """x N(0, 1) with a per-row offset and scale, gamma, integer-valued dy and dy2 in [-8, 8] (dbeta is then an exact sum),
    drawn where they are used."""
    g = torch.Generator(device=device).manual_seed(zlib.crc32(repr(("ln", M, D)).encode()))
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    x = rn(M, D) * (0.5 + torch.rand(M, 1, generator=g, device=device)) + rn(M, 1)
    gamma = 1 + 0.1 * rn(D)
    dy = torch.randint(-8, 9, (M, D), generator=g, device=device).float()
    dy2 = torch.randint(-8, 9, (M, D), generator=g, device=device).float()
    return x, gamma, dy, dy2


def ln_ref(x, gamma, dy, dtype):
    """(dx, dgamma, dbeta) of LayerNorm(eps 1e-5) over the last dimension in `dtype`, where the tensors live."""
    xd = x.to(dtype).requires_grad_(True)
    gd = gamma.to(dtype).requires_grad_(True)
    bd = torch.zeros_like(gd).requires_grad_(True)
    y = torch.nn.functional.layer_norm(xd, (x.shape[-1],), gd, bd, 1e-5)
    return torch.autograd.grad(y, (xd, gd, bd), dy.to(dtype))


# ================================================================================================ GroupNorm partials
# gn_blocks: 4 sequences a block, 1024 blocks at most.  S = B * N -> (B, N)
GN_S = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (1, 5), 4095: (5, 819), 4096: (2, 2048), 4097: (17, 241), 8193: (3, 2731)}
# kernel group -> (L, Cout, every tensor bf16, TECM_GN_BWD_SPLIT, the path tecm_gn_bwd_path names)
GN_KERNELS = {
    "rows": (6, 64, False, None, "gn_gelu_bwd_kernel<1>"),
    "reg4": (48, 64, False, None, "gn_gelu_bwd_reg<1,4,9,false,false,false>"),
    "reg8": (96, 64, False, None, "gn_gelu_bwd_reg<1,8,9,false,false,false>"),
    "oct": (40, 64, True, "0", "gn_gelu_bwd_reg16<1,3>"),
    "split64": (16, 64, True, None, "gn_bwd_sums16_kernel<1>+gn_bwd_apply16_kernel<1>"),
    "split128": (24, 128, True, None, "gn_bwd_sums16_kernel<2>+gn_bwd_apply16_kernel<2>"),
}
# the split pair deals (sample, node group) items of 10 (Cout 64) / 5 (Cout 128) nodes over min(ceil(B * N / 4), 1024) blocks:
# N either side of one group, with more items than blocks -- (B, N) -> items B * ceil(N / group) > 1024 blocks
GN_SPLIT_ITEMS = {"split64": ((1025, 9), (1025, 10), (600, 11)), "split128": ((1025, 4), (1025, 5), (600, 6))}


def gn_items(kernel, B, N):
    group = 10 if kernel == "split64" else 5
    return B * ((N + group - 1) // group), min((B * N + 3) // 4, 1024)


def gn_case_inputs(kernel, B, N, device):
    """(y, dact, gamma, beta) on the device, fp32 tensors holding bf16-representable values where the kernel reads bf16."""
    L, Cout, all16, _, _ = GN_KERNELS[kernel]
    CT = 3 * Cout
    g = torch.Generator(device=device).manual_seed(zlib.crc32(repr(("gn", kernel, B, N)).encode()))
    y = torch.randn(B, L, N, CT, generator=g, device=device)
    dact = torch.randn(B, L, N, CT, generator=g, device=device)
    if all16:
        y, dact = y.bfloat16().float(), dact.bfloat16().float()
    gc = gen("gn-affine", Cout)
    gamma, beta = 1 + 0.1 * torch.randn(CT, generator=gc), 0.1 * torch.randn(CT, generator=gc)
    return y, dact, gamma.to(device), beta.to(device)


def gn_ref(y, dact, gamma, beta, Cout):
    """float64 GroupNorm(1, Cout) + GELU per branch, where the tensors live: (dy, dgamma, dbeta, column sums of dy), written
    out -- elementwise operations and plain sums only.  (torch's own group_norm backward on the device returned parameter
    gradients half the size of these at 4095 sequences; the host test holds this function to torch's autograd on the CPU.)"""
    B, L, N, CT = y.shape
    yd, dd = y.double().view(B, L, N, 3, Cout), dact.double().view(B, L, N, 3, Cout)
    g, b = gamma.double().view(3, Cout), beta.double().view(3, Cout)
    grp = (1, 4)                                                   # one (sample, node, branch) group: L steps x Cout channels
    mean = yd.mean(grp, keepdim=True)
    rstd = 1.0 / torch.sqrt(((yd - mean) ** 2).mean(grp, keepdim=True) + 1e-5)
    yhat = (yd - mean) * rstd
    z = yhat * g + b
    dz = dd * (0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))
    gg, gb = (dz * yhat).sum((0, 1, 2)).reshape(CT), dz.sum((0, 1, 2)).reshape(CT)
    dh = dz * g
    gy = (rstd * (dh - dh.mean(grp, keepdim=True) - yhat * (dh * yhat).mean(grp, keepdim=True))).reshape(B, L, N, CT)
    return gy, gg, gb, gy.sum((0, 1, 2))


# ================================================================================================ Huber
HUBER_BLOCK_CAP = 1024               # tecm_huber_fwd_bwd{,_strided}: min(ceil(n / 256), 1024) blocks of 256 threads
HUBER_N = (1, 255, 256, 257, 256 * HUBER_BLOCK_CAP - 1, 256 * HUBER_BLOCK_CAP, 256 * HUBER_BLOCK_CAP + 1, 300001)
HUBER_STRIDED = [(4, H, N) for H in (1, 12, 24) for N in (1, 63, 2911)]         # (B, H, N); 4 x 24 x 2911 is past the cap
HUBER_GRAD_SCALES = (1.0, 0.125, 4.0)


def huber_exact_inputs(shape, seed):
    """(pred, target, residual): residuals are multiples of 0.25 in [-3, 3], targets multiples of 0.25 in [-4, 4], so pred -
    target is exact in fp32; with delta = 1 every loss term is a multiple of 2^-5 of at most 2.5, and the sum over up to
    300001 of them (mean 1.1) stays below 2^19: exact in any order."""
    g = gen("huber", shape, seed)
    r = torch.randint(-12, 13, shape, generator=g).float() * 0.25
    t = torch.randint(-16, 17, shape, generator=g).float() * 0.25
    return t + r, t, r


def huber_exact_ref(r, n, grad_scale):
    """(exact mean loss as a float, dpred fp32): dpred = clamp(r, -1, 1) * fl(grad_scale / n), one correctly rounded product."""
    a = r.double().abs()
    loss = torch.where(a <= 1, 0.5 * a * a, a - 0.5).sum().item() / n
    gs = float(np.float32(grad_scale) / np.float32(n))
    return loss, (r.double().clamp(-1, 1) * gs).float()


def ulps32(got, exact):
    """Distance of an fp32 value from a real number in units of the fp32 spacing at that number."""
    e = np.float32(exact)
    return abs(float(got) - exact) / float(np.spacing(np.abs(e)))


# ================================================================================================ clip norm + AdamW
NORM_BLOCKS = 512                    # TECM_NORM_BLOCKS: the norm pass runs min(ceil(n / 4 / 256), 512) blocks
ADAMW_BLOCK_CAP = 2048               # the update min(ceil(n / 4 / 256), 2048)
ADAMW_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 1024 * NORM_BLOCKS - 1, 1024 * NORM_BLOCKS, 1024 * NORM_BLOCKS + 3,
           1024 * ADAMW_BLOCK_CAP + 1029)
# (zero_grad, max_norm, weight_decay, step, grad_scale), cycled over ADAMW_N
ADAMW_OPTS = ((1, 1.0, 0.01, 1, 1.0), (0, 0.0, 0.0, 1000, 0.125), (1, 1.0, 0.0, 1000, 0.5), (0, 1.0, 0.01, 1, 0.125),
              (1, 0.0, 0.01, 1000, 1.0), (0, 1.0, 0.0, 1, 1.0))
ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
ADAMW_RTOL, ADAMW_ATOL = 2e-6, 1e-8  # test_flat_adamw_state_dict_round_trips_through_torch_adamw


def adamw_inputs(n):
    """(p, g, exp_avg, exp_avg_sq): N(0, 1) parameters and integer-valued gradients in [-8, 8] (the sum of squares is exact).
    The moments are chosen so that fp32 can meet an absolute tolerance of 1e-8 at all, whoever computes: exp_avg carries the
    sign of its gradient -- b1 * m + (1 - b1) * g then never cancels, where the half-ulp roundings of two products of size
    0.1 .. 0.8 (4e-9 .. 3e-8) would be the whole result -- and exp_avg_sq is at least 1e-3, which bounds the update at
    lr / bc1 * 1.25 / sqrt(1e-3 / bc2) <= 0.032 for both step counts used: the five fp32 roundings on the way to it, 1.5e-7 of
    it, stay below 1e-8 where p - update cancels."""
    g = gen("adamw", n)
    p = torch.randn(n, generator=g)
    grad = torch.randint(-8, 9, (n,), generator=g).float()
    m = 0.1 * torch.randn(n, generator=g).abs() * torch.where(grad < 0, -1.0, 1.0)
    return p, grad, m, 1e-3 + 0.01 * torch.rand(n, generator=g)


def adamw_ref(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale, step):
    """One clip_grad_norm_(max_norm) + AdamW step in float64, where the tensors live: (norm, p, m, v)."""
    p, g, m, v = p.double(), g.double() * grad_scale, m.double(), v.double()
    norm = math.sqrt(float((g * g).sum()))
    if max_norm > 0:
        g = g * min(1.0, max_norm / (norm + 1e-6))
    p = p * (1 - lr * weight_decay)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    p = p - (lr / (1 - beta1 ** step)) * m / (v.sqrt() / math.sqrt(1 - beta2 ** step) + eps)
    return norm, p, m, v


def exact_norm(g_int, grad_scale):
    """fl(sqrt(exact sum of squares)) * |grad_scale| for integer-valued gradients, as a float."""
    ss = int((g_int.to(torch.int64) ** 2).sum())
    return float(np.float32(math.sqrt(ss))) * abs(grad_scale)


# ================================================================================================ checksum
CSUM_BLOCKS = 256
CSUM_N = (1, 255, 256, 257, 256 * CSUM_BLOCKS - 1, 256 * CSUM_BLOCKS, 256 * CSUM_BLOCKS + 1)
CSUM_WORLDS = (1, 8)
