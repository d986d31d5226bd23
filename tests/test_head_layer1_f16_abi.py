"""CPU: manet_head_layer1_object_f16 (head_act="f16", layer 1's per-object half in one launch) is declared, bound and exported,
and refuses bad arguments before anything reaches a device; ops.head_layer1_object_f16 refuses what it cannot run."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NAME = "manet_head_layer1_object_f16"


@pytest.fixture(scope="module")
def lib():
    from cvpr2020_manet_amd import _lib
    return _lib.load()


def test_symbol_is_declared_bound_and_exported(lib):
    from cvpr2020_manet_amd import _lib
    header = open(os.path.join(ROOT, "include", "manet_hip.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % NAME, header)
    assert m, "%s is not declared in include/manet_hip.h" % NAME
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == len(params) == 15
    for p, a in zip(params, args):  # pointers and the stream as void *, the rest as int
        assert a is (ctypes.c_void_p if ("*" in p or "manet_stream_t" in p) else ctypes.c_int), (p, a)
    assert getattr(lib, NAME).argtypes == args
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


def _refused(lib, rc, *words):
    msg = lib.manet_last_error_string().decode()
    assert rc == -1 and all(w in msg for w in words), (rc, msg)


def test_entry_point_refuses_bad_arguments_before_any_launch(lib):
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16  # a 16-byte aligned host address: never dereferenced
    f = getattr(lib, NAME)

    def call(planes=p, n=3, Cp=3, h=8, w=12, dw_weight=p, dw_bias=None, bn_scale=None, bn_shift=None, wpk=p, b2=p, term=p,
             relu_out=1, out=p):
        return f(planes, n, Cp, h, w, dw_weight, dw_bias, bn_scale, bn_shift, wpk, b2, term, relu_out, out, None)

    _refused(lib, call(planes=None), "planes is NULL")
    _refused(lib, call(dw_weight=None), "dw_weight is NULL")
    _refused(lib, call(wpk=None), "wpk is NULL")
    _refused(lib, call(b2=None), "b2 is NULL")
    _refused(lib, call(out=None), "out is NULL")
    _refused(lib, call(n=0), "n=0")
    _refused(lib, call(n=-2), "n=-2")
    _refused(lib, call(Cp=0), "Cp=0")
    _refused(lib, call(Cp=5), "Cp=5")
    _refused(lib, call(w=13), "w=13", "even")
    _refused(lib, call(h=9, w=12), "h*w=108", "multiple of 8")
    _refused(lib, call(h=3, w=4), "h*w=12", "multiple of 8")
    _refused(lib, call(h=2, w=2), "h*w=4", "at least 8")
    _refused(lib, call(term=p + 8), "term", "16-byte aligned")
    _refused(lib, call(out=p + 8), "out", "16-byte aligned")
    _refused(lib, call(wpk=p + 4), "wpk", "16-byte aligned")
    # (term may be NULL: nothing is added; the NULL forms of dw_bias / bn_scale / bn_shift are 0 / 1 / 0)


def test_op_refuses_a_plain_weight_and_cpu_tensors():
    from cvpr2020_manet_amd import ops
    per, dw = torch.zeros(2, 3, 8, 12), torch.zeros(3, 1, 7, 7)
    with pytest.raises(TypeError, match="HalfWeight"):
        ops.head_layer1_object_f16(per, dw, None, None, None, torch.zeros(3, 256), torch.zeros(256))
    weight = object.__new__(ops.HalfWeight)  # (packing needs a device; the refusal comes before the weight is read)
    weight.cin, weight.packed = 3, None
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.head_layer1_object_f16(per, dw, None, None, None, weight, torch.zeros(256))
    assert ops.head_layer1_object_f16_ok(per) and ops.head_layer1_object_f16_ok(torch.zeros(1, 4, 1, 8))
    for shape in ((2, 5, 8, 12), (2, 3, 8, 13), (2, 3, 9, 12), (2, 3, 2, 2), (0, 3, 8, 12)):
        assert not ops.head_layer1_object_f16_ok(torch.zeros(shape)), shape
