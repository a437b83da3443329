"""CPU: which kernel the MED head's entry points take for a shape (falnet_med_head_kernel_name), held to a table recorded from the library
before the choice was written once (csrc/med_head.hip: choose_head_fwd / choose_head_bwd_nhwc).  The name function and the launches ask
the same chooser, so this table is also what runs; tests/test_gpu_head.py shows that every kernel in it is run."""
import ctypes as C

import pytest

from fal_net_amd import _lib as L

NAMES = {"f": "med_head_fwd_kernel", "l": "med_head_fwd_lds_kernel", "s": "med_head_fwd_lds2_kernel", "S": "med_head_fwd_lds2_kernel<512 threads>",
         "p": "med_head_bwd_kernel<planar>", "n": "med_head_bwd_kernel<nhwc>", "L": "med_head_bwd_lds_kernel", "t": "med_head_bwd_lds2_kernel",
         "T": "med_head_bwd_lds2_kernel<512 threads>", "w": "med_head_bwd_wave_kernel"}
WIDTHS = (3, 4, 40, 77, 252, 256, 260, 512, 1020, 1024, 1028, 1242, 1280, 1984, 1988, 2048, 2049, 2052, 2100, 8112)
PLANES = (2, 49, 120, 121, 128)
DTYPES = (L.F32, L.BF16, L.F16)
# one letter of NAMES per width of WIDTHS; rows: N <= 120 (the register plane table of the second-generation kernels reaches N + 7), N >= 121
FWD = {120: "lsslssssssSlSSSSffff", 128: "lllllllllllllfffffff"}        # pass 0, every dtype
PLANAR = {120: "p" * 20, 128: "p" * 20}                                  # pass 1, every dtype
NHWC_F32 = {120: "LttLttttttTnTTTTnnnn", 128: "LLLLLLLLLLwnwwnnnnnn"}   # pass 2
NHWC_16 = {120: "LttLttttttwnwwTTnnnn", 128: "LLLLLLLLLLwnwwnnnnnn"}    # pass 2, bf16 and f16: the wave-neighbour kernel where it applies
TABLE = {(0, dt): FWD for dt in DTYPES}
TABLE.update({(1, dt): PLANAR for dt in DTYPES})
TABLE.update({(2, L.F32): NHWC_F32, (2, L.BF16): NHWC_16, (2, L.F16): NHWC_16})
CASES = [(pas, dt, N) for (pas, dt) in sorted(TABLE) for N in PLANES]


def _name(pas, dt, N, W):
    buf = C.create_string_buffer(96)
    rc = L.lib().falnet_med_head_kernel_name(pas, dt, N, W, buf, 96)
    return rc, buf.value.decode()


def test_the_table_names_every_head_kernel():
    assert len(NAMES) == 10 and len(set(NAMES.values())) == 10
    assert {c for rows in TABLE.values() for row in rows.values() for c in row} == set(NAMES)
    assert all(len(row) == len(WIDTHS) for rows in TABLE.values() for row in rows.values())


@pytest.mark.parametrize("pas,dt,N", CASES)
def test_kernel_choice_is_the_recorded_one(pas, dt, N):
    row = TABLE[(pas, dt)][120 if N <= 120 else 128]
    got = [_name(pas, dt, N, W) for W in WIDTHS]
    assert got == [(0, NAMES[c]) for c in row]


@pytest.mark.parametrize("pas", (0, 1, 2))
@pytest.mark.parametrize("dt", DTYPES)
def test_refusals_are_the_recorded_ones(pas, dt):
    """N = 1, N = 129, and W = 8113: the first width the limit rejects, (W + 3) 20 + 1536 > 163 840."""
    for N, W, msg in ((1, 40, "med_head: N=1 outside [2,128]"), (129, 40, "med_head: N=129 outside [2,128]"), (49, 8113, "med_head: W=8113 too wide for LDS")):
        assert _name(pas, dt, N, W)[0] == -1
        assert L.lib().falnet_last_error().decode() == msg
    assert _name(pas, dt, 49, 8112)[0] == 0
