"""Packed feature rows on the CPU (include/wab.h, WAB_HAS_PACKED_FEATURES): the header and its
ctypes mirror, the format as wab_gym_amd.features states it in NumPy, and the Python argument
checks that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import packed_cases as pkc
import policy_grad_cases as pgc
from wab_gym_amd import _lib, features, policy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wab.h")
PAIRS = (("wab_policy_evaluate_packed", "wab_policy_evaluate_gather"),
         ("wab_policy_grad_packed", "wab_policy_grad_gather"),
         ("wab_policy_grad_ppo_packed", "wab_policy_grad_ppo_gather"))


def declared_args(name):
    """The argument list of a function the header declares, one 'type name' string per argument."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_defines_the_format_and_keeps_the_abi():
    src = open(HEADER).read()
    assert re.search(r"^#define WAB_HAS_PACKED_FEATURES 1\b", src, flags=re.M)
    abi = int(re.search(r"^#define WAB_ABI_VERSION (\d+)", src, flags=re.M).group(1))
    assert abi == _lib.ABI_VERSION == 14
    for name in ("wab_feature_bits_pitch", "wab_features_pack", "wab_features_unpack", "wab_rollout_policy_packed") \
            + tuple(p for p, _ in PAIRS):
        assert name in _lib.EXPORTED and re.fullmatch(r"wab_[a-z_]+", name), name


def test_packed_calls_take_their_gather_twins_arguments():
    for packed, gather in PAIRS:
        a, b = declared_args(packed), declared_args(gather)
        assert b[1] == "const float* features" and a[1] == "const uint32_t* feature_bits", (packed, a[1], b[1])
        assert a[:1] + a[2:] == b[:1] + b[2:], packed
    a, b = declared_args("wab_rollout_policy_packed"), declared_args("wab_rollout_policy")
    i = b.index("float* features")
    assert a[i] == "uint32_t* feature_bits" and a[:i] + a[i + 1:] == b[:i] + b[i + 1:]


def test_pitch_is_four_dwords_per_128_features():
    for F in pkc.PITCH_F:
        assert features.bits_pitch(F) == pkc.pitch(F) == 4 * int(np.ceil(F / 128.0)), F
    assert [features.bits_pitch(F) for F in (1, 128, 129, 449, 1 << 20)] == [4, 4, 8, 16, 32768]
    for F in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError):
            features.bits_pitch(F)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libwab_hip.so not built")
    L = _lib.load()
    for F in pkc.PITCH_F + (1 << 20,):
        assert L.wab_feature_bits_pitch(F) == pkc.pitch(F), F
    for F in (0, -1, (1 << 20) + 1):
        assert L.wab_feature_bits_pitch(F) == -1 and b"in_features" in L.wab_last_error()


def test_reference_round_trip_on_the_golden_rows():
    x = np.load(os.path.join(REPO, "tests", "golden", "pragmatic.npz"))["features"]
    assert x.dtype == np.float32 and x.shape[1] == 449
    u = x.view(np.uint32)
    assert ((u == 0) | (u == 0x3F800000)).all()  # binary, and no -0.0
    assert features.nonbinary_reference(x) == 0
    bits = features.pack_reference(x)
    assert bits.dtype == np.int32 and bits.shape == (x.shape[0], 16)
    back = features.unpack_reference(bits, 449)
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), u)
    # the format, element by element: feature k is bit k & 31 of dword k >> 5; the pad bits are zero
    ub = bits.view(np.uint32)
    for k in (0, 1, 31, 32, 33, 200, 448):
        assert np.array_equal((ub[:, k >> 5] >> np.uint32(k & 31)) & 1, u[:, k] != 0), k
    assert not (ub[:, 14] >> np.uint32(1)).any() and not ub[:, 15].any()  # bits 449 .. 511
    assert int(np.unpackbits(ub.view(np.uint8)).sum()) == int((u != 0).sum())
    # the pad bits are ignored by the unpack, and -0.0, 0.5 and NaN set their bit and are counted
    dirty = ub.copy()
    dirty[:, 14] |= np.uint32(0xFFFFFFFE)
    dirty[:, 15] = 0xFFFFFFFF
    assert np.array_equal(features.unpack_reference(dirty.view(np.int32), 449), back)
    y = np.zeros((2, 33), np.float32)
    y[0, 0], y[0, 32], y[1, 5], y[1, 6] = -0.0, 0.5, np.nan, 1.0
    assert features.nonbinary_reference(y) == 3
    assert np.array_equal(features.pack_reference(y).view(np.uint32),
                          np.array([[1, 1, 0, 0], [0x60, 0, 0, 0]], np.uint32))
    for F in (1, 31, 32, 33, 128):
        r = pkc.binary_rows(F, 65)
        assert np.array_equal(features.unpack_reference(features.pack_reference(r), F), r)


def test_python_checks_refuse_wrong_packed_tensors():
    net = pkc.NET_REF
    P = pkc.pitch(net[0])
    shape = policy.shape_of(pgc.state_dict(net))
    ok = torch.zeros((6, P), dtype=torch.int32)
    a = torch.zeros(6, dtype=torch.int8)
    assert policy.check_rows(shape, ok, actions=a) == 6
    assert policy.check_rows(shape, ok.view(2, 3, P), actions=a.view(2, 3)) == 6
    assert features.check_bits(ok, net[0], "cpu") == 6
    wrong = [torch.zeros((6, P + 4), dtype=torch.int32),          # a wrong P
             torch.zeros((6, P - 4), dtype=torch.int32),
             torch.zeros((6, 2 * P), dtype=torch.int32)[:, ::2],  # not contiguous
             torch.zeros((P,), dtype=torch.int32),                # no row dimension
             torch.zeros((6, P), dtype=torch.int64),              # a wrong dtype
             torch.zeros((6, P), dtype=torch.uint8)]
    for bad in wrong:
        with pytest.raises(ValueError):
            policy.check_rows(shape, bad)
    for bad in wrong[:3] + wrong[4:]:
        with pytest.raises(ValueError):
            features.check_bits(bad, net[0])
    with pytest.raises(ValueError):  # a wrong device
        features.check_bits(ok, net[0], "cuda:0")
    with pytest.raises(ValueError):  # the per-row tensors follow the bits' leading shape
        policy.check_rows(shape, ok, actions=torch.zeros(5, dtype=torch.int8))
    for call in (features.pack_features, lambda x: features.unpack_features(x, net[0])):
        with pytest.raises(ValueError):  # the kernels run on a GPU: host tensors are refused
            call(ok if call is not features.pack_features else torch.zeros((6, net[0])))
    with pytest.raises(ValueError):
        features.pack_features(torch.zeros((6, 8), dtype=torch.float64))
