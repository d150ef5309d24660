"""CPU side of the bf16x3 precision: the dtype code in the header and in _lib, the library version, the host entry points that take it"""
import os
import re

import pytest
import torch

from zeroshotsemanticsegmentation_amd import _lib as L
from zeroshotsemanticsegmentation_amd import models, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dtype_code_in_header_and_lib():
    src = open(os.path.join(ROOT, "include", "szn.h")).read()
    m = re.search(r"enum\s*\{\s*SZN_F32 = 0, SZN_BF16 = 1, SZN_F16 = 2, SZN_BF16X3 = (\d+)\s*\}", src)
    assert m and int(m.group(1)) == 3
    assert L.SZN_BF16X3 == 3


def test_library_version():
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libszn_hip.so not built")
    assert L.load().szn_version() >= 102


def test_train_cli_accepts_bf16x3():
    args = train.build_parser().parse_args(["--precision", "bf16x3"])
    assert args.precision == "bf16x3"


def test_set_precision_bf16x3_keeps_fp32_storage():
    m = models.FCN32s(20)
    eng = m._engine
    m.set_precision("bf16x3")
    assert eng.dtype == torch.float32 and eng.bf16x3 and eng.precision == "bf16x3"
    assert eng._gemm_code("conv3_2") == L.SZN_BF16X3 and eng._gemm_code("fc6") == L.SZN_BF16X3
    assert eng._gemm_code("head") == L.SZN_F32 and eng._gemm_code(None) == L.SZN_F32      # head / skip layers stay exact
    m.set_precision(torch.float32)
    assert not eng.bf16x3 and eng._gemm_code("conv3_2") == L.SZN_F32
    with pytest.raises(L.SznError):
        m.set_precision("bf16")
