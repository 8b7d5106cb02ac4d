"""CPU: the device code the kernels share is stated once.  A text scan of minddet_amd/csrc: the bf16 conversions, the packed ReLU, the
buffer-descriptor flag word and the vector typedefs live in device.h, the delta-to-box arithmetic in box_codec.h, the training losses'
block sums, focal terms, strip staging and ownership rule in loss_common.h, the integer wave and workgroup primitives (scans, ballot
ranks) in workgroup.h, the gather-form Gaussian heat map in heatmap.h, the anchor mask's kernels (one set for md_anchor_mask and
md_pp_anchor_mask) in ppreader.hip, and no other file spells any of them again (a new kernel includes the header instead of copying
the file before it)."""
import glob
import os

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minddet_amd", "csrc")
SRC = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))}
HIP = sorted(n for n in SRC if n.endswith(".hip"))

# text that marks a private copy -> the one header that may hold it
ONLY_IN = {
    "v_cvt_pk_bf16_f32": "device.h",     # fp32 pair -> packed bf16
    "v_pk_max_i16": "device.h",          # packed ReLU
    "0x00020000": "device.h",            # gfx950 buffer-descriptor flag word
    "0x7fffu +": "device.h",             # software round-to-nearest-even
    "ext_vector_type": "device.h",       # vector typedefs
    "fminf(fmaxf(dw": "box_codec.h",     # delta-to-box decode
    "__shfl_down(v[e]": "loss_common.h",       # the losses' fixed-order block sums
    "1.0 - 1e-4": "loss_common.h",             # the clipped sigmoid of the focal terms
    "(pred > target)": "loss_common.h",        # the sign of an L1 term
    "elems / 8": "loss_common.h",              # the 16-byte staging of a dense kernel's strip
    "hi[i] <= lo[j]": "loss_common.h",         # each gradient element has one owner
    "__shfl_up(": "workgroup.h",               # the 64-lane inclusive scan
    "(1ull << lane) - 1ull": "workgroup.h",    # a lane's rank in a ballot
    "exp(-((double)dx": "heatmap.h",           # the float64 Gaussian of a heat map
    "2.0 * sigma * sigma": "heatmap.h",        # its denominator
    "d[C3 * nx + C2]": "ppreader.hip",         # the anchor mask's 4-corner box sum
    "acc += d[": "ppreader.hip",               # its column cumsum
}


def test_every_translation_unit_was_read():
    assert len(HIP) >= 15 and {"device.h", "box_codec.h", "aot.h", "loss_common.h", "workgroup.h", "heatmap.h"} <= set(SRC)


@pytest.mark.parametrize("text", list(ONLY_IN), ids=[t.strip("( +") for t in ONLY_IN])
def test_shared_device_code_is_stated_once(text):
    home = ONLY_IN[text]
    assert text in SRC[home], f"{home} no longer holds {text!r}: move this test's entry with it"
    assert [n for n in SRC if n != home and text in SRC[n]] == []


def test_aot_header_is_host_only():
    assert "__device__" not in SRC["aot.h"] and "__builtin_amdgcn" not in SRC["aot.h"]
    users = [n for n in HIP if "MD_BUFFER_STORE_B128" in SRC[n] or "MD_WAVE_LDS_ORDER" in SRC[n]]
    assert users and all('#include "device.h"' in SRC[n] for n in users)
