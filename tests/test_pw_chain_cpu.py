"""CPU: the ABI of include/minddet_hip_chain.h without a GPU -- header, symbol, Makefile, the argument checks of md_pw_chain before any
device call (the single-defect calls and its documented refusals, made with the kit of tests/abi_derive.py), and the packs
graphs.ResNet makes for it."""
import ctypes as C
import os

import pytest

from minddet_amd import graphs, nn_ops
from tests import abi_header as ah
from tests.abi_cases_chain import CASES
from tests.abi_derive import ITEM, Call, lib_handle, rc, refuse_single_defects, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 2


def test_chain_header_declares_the_symbol_and_the_main_header_does_not():
    ch = ah.header("minddet_hip_chain.h")
    main = ah.header("minddet_hip.h")
    assert ah.aot_symbols(ch) == ["md_pw_chain"] and '#include "minddet_hip.h"' in ch
    assert "md_pw_chain" not in ah.aot_symbols(main)
    assert {c.sym for c in CASES} == {"md_pw_chain"}
    assert "minddet_hip_chain.h" in open(os.path.join(ROOT, "minddet_amd", "csrc", "Makefile")).read()
    assert hasattr(lib_handle(), "md_pw_chain")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_without_a_device(case):
    refuse_single_defects("abi_cases_chain", case)


def test_other_channel_counts_and_shapes_return_2():
    for e in (shape(0, (1, 3, 5, 64)), shape(0, (1, 3, 5, 256)),        # t2: other mid channels, a channel slice of a wider tensor
              shape(1, (1, 3, 5, 256)), shape(1, (1, 3, 5, 1024)),      # res
              shape(6, (1, 3, 5, 1024)), shape(7, (1, 3, 5, 256)),      # outputs wider than the layer (a channel-concat buffer)
              shape(2, (512, 192)), shape(2, (256, 128)), shape(4, (128, 576)), shape(4, (64, 512)),
              shape(3, (256,), "float32"), shape(5, (64,), "float32"),
              shape(1, (1, 3, 4, 512)), shape(6, (2, 3, 5, 512)), shape(7, (1, 5, 3, 128))):
        assert rc(CASES[0], e) == ARG


class _Aliased(Call):
    """Call whose operand `dst` starts `shift` bytes into operand `src`'s host block"""

    def __init__(self, case, dst, src, shift):
        super().__init__(case)
        self.dst, self.src, self.shift = dst, src, shift

    def run(self, lib):
        ops = self.case.operands
        n = len(ops)
        numel = lambda s: int(__import__("math").prod(s))
        sizes = [ITEM[t.dtype] * numel(t.shape) + 64 for t in ops]
        arena = (C.c_char * (2 * sum(sizes)))()
        base, offs, off = C.addressof(arena), [], 0
        for s in sizes:
            offs.append(off)
            off += 2 * s           # room for an aliased output to run past its source
        offs[self.dst] = offs[self.src] + self.shift
        params = (C.c_void_p * n)(*[base + o for o in offs])
        ndims = (C.c_int * n)(*[len(t.shape) for t in ops])
        keep = [(C.c_int64 * len(t.shape))(*t.shape) for t in ops]
        shapes = (C.POINTER(C.c_int64) * n)(*[C.cast(k, C.POINTER(C.c_int64)) for k in keep])
        dtypes = (C.c_char_p * n)(*[t.dtype.encode() for t in ops])
        return lib.md_pw_chain(n, params, ndims, shapes, dtypes, None, None)


def test_outputs_overlapping_an_input_or_each_other_return_2():
    lib = lib_handle()
    case = CASES[0]
    res_bytes, t2_bytes = 15 * 512 * 2, 15 * 128 * 2
    # y in place on the residual, y one pixel into it, y ending inside it; t1 in place on t2; y on t2; t1 on res; t1 inside y
    for dst, src, shift in ((6, 1, 0), (6, 1, 1024), (6, 1, res_bytes - 16), (7, 0, 0), (7, 0, t2_bytes - 16), (6, 0, 0), (7, 1, 2048),
                            (7, 6, 0), (7, 6, res_bytes - 2)):
        assert _Aliased(case, dst, src, shift).run(lib) == ARG, (dst, src, shift)


def test_resnet_packs_a_chain_for_the_inner_identity_blocks_of_stage_2_only():
    for depth, layers in ((50, [3, 4, 6, 3]), (101, [3, 4, 23, 3])):
        bb = graphs.ResNet(depth=depth).to("cpu")
        assert sorted(bb._chains) == [(1, 1), (1, 2)], (depth, sorted(bb._chains))    # b2 -> b3 and b3 -> b4; the first and the last block keep their path
        for (si, bi), pk in bb._chains.items():
            assert pk.w3 is bb.stages[si][bi].conv3.packed.w and pk.w1 is bb.stages[si][bi + 1].conv1.packed.w
    st = graphs.ResNet(depth=50).to("cpu").stages
    assert nn_ops.pack_pw_chain(st[2][1].conv3.packed, st[2][2].conv1.packed) is None       # stage 3: 256 / 1024 channels
    assert nn_ops.pack_pw_chain(st[1][0].conv3.packed, st[1][1].conv1.packed) is not None   # (the shapes fit; the first block's residual is its downsample conv)
    assert graphs.ResNet(depth=18).to("cpu")._chains == {}
