"""Packed feature rows: 1 bit per feature (include/wab.h, WAB_HAS_PACKED_FEATURES).

A PragmaticObsWrapper row is a one-hot layout, every float 0.0 or 1.0.  A packed row of F features
is P = 4 * ceil(F / 128) little-endian dwords (a multiple of 16 bytes): feature k is bit k & 31 of
dword k >> 5, and bits F .. 32 P - 1 are zero.  Tensors are int32 [..., P] (torch has no uint32
arithmetic; the bits are the same).

    bits = pack_features(features)                 # [T, B, F] float32 -> [T, B, P] int32, on the device
    policy.ppo_loss_and_grad(bits, ...)            # the packed calls, by the dtype
    unpack_features(bits, F)                       # -> float32, exactly 0.0 / 1.0

`pack_reference` / `unpack_reference` state the format in NumPy.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def bits_pitch(F):
    """P, the dwords of a packed row of F features (wab_feature_bits_pitch)."""
    F = int(F)
    if not 1 <= F <= 1 << 20:
        raise ValueError("in_features outside [1, 2^20]: %d" % F)
    return 4 * ((F + 127) // 128)


def pack_reference(x):
    """NumPy statement of wab_features_pack: x [..., F] float32 -> int32 [..., P]; the bit is set
    iff the float's bit pattern is not 0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    F = x.shape[-1]
    P = bits_pitch(F)
    on = np.zeros(x.shape[:-1] + (32 * P,), dtype=np.uint8)
    on[..., :F] = x.view(np.uint32) != 0
    return np.packbits(on, axis=-1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


def unpack_reference(bits, F):
    """NumPy statement of wab_features_unpack: int32 (or uint32) [..., P] -> float32 [..., F] of
    exactly 0.0 / 1.0; the bits from F on are ignored."""
    bits = np.ascontiguousarray(bits)
    if bits.dtype not in (np.int32, np.uint32) or bits.shape[-1] != bits_pitch(F):
        raise ValueError("bits must be int32 [..., %d] for F = %d" % (bits_pitch(F), F))
    on = np.unpackbits(bits.view(np.uint32).astype("<u4").view(np.uint8), axis=-1, bitorder="little")
    return on[..., :F].astype(np.float32)


def nonbinary_reference(x):
    """The count wab_features_pack adds to `nonbinary`: elements whose pattern is neither
    0x00000000 nor 0x3F800000 (-0.0 and NaN count)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return int(np.count_nonzero((u != 0) & (u != 0x3F800000)))


def check_bits(bits, F, device=None):
    """The checks of a packed tensor that need no device: int32, contiguous, [..., P] for F
    features, on `device` where one is given.  Returns the number of rows."""
    import torch

    P = bits_pitch(F)
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32:
        raise ValueError("packed features must be an int32 torch tensor [..., %d]" % P)
    if bits.dim() < 1 or bits.shape[-1] != P:
        raise ValueError("packed features of %d features have %d dwords per row, not shape %s"
                         % (F, P, tuple(bits.shape)))
    if not bits.is_contiguous():
        raise ValueError("packed features must be contiguous")
    if device is not None and bits.device != torch.device(device):
        raise ValueError("packed features must be on %s, not %s" % (device, bits.device))
    n = 1
    for k in bits.shape[:-1]:
        n *= int(k)
    return n


def _stream(x):
    import torch

    return torch.cuda.current_stream(x.device).cuda_stream


def pack_features(x, out=None, check=True):
    """x [..., F] float32, contiguous, on a GPU -> int32 [..., P] (wab_features_pack, one launch on
    the current stream).  check=True reads the device's count of elements that are neither 0.0 nor
    1.0 (this synchronises) and raises ValueError when it is not 0; check=False neither counts
    nor synchronises."""
    import torch

    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 1 or not x.is_contiguous():
        raise ValueError("features must be a contiguous float32 torch tensor [..., F]")
    if x.device.type != "cuda":
        raise ValueError("features must be on a GPU, not %s" % (x.device,))
    F = int(x.shape[-1])
    P = bits_pitch(F)
    lead = tuple(x.shape[:-1])
    if out is None:
        out = torch.empty(lead + (P,), dtype=torch.int32, device=x.device)
    elif check_bits(out, F, x.device) is None or tuple(out.shape[:-1]) != lead:
        raise ValueError("out must have shape %s" % (lead + (P,),))
    n = out.numel() // P
    count = torch.zeros(1, dtype=torch.int64, device=x.device) if check else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().wab_features_pack(x.data_ptr(), n, F, out.data_ptr(),
                                                 None if count is None else count.data_ptr(), _stream(x)),
                   "wab_features_pack")
    if check:
        bad = int(count.item())
        if bad:
            raise ValueError("pack_features: %d elements are neither 0.0 nor 1.0 (a packed row keeps one bit per "
                             "feature)" % bad)
    return out


def unpack_features(bits, F, out=None):
    """int32 [..., P] on a GPU -> float32 [..., F] of exactly 0.0 / 1.0 (wab_features_unpack, one
    launch on the current stream)."""
    import torch

    F = int(F)
    n = check_bits(bits, F)
    if bits.device.type != "cuda":
        raise ValueError("packed features must be on a GPU, not %s" % (bits.device,))
    lead = tuple(bits.shape[:-1])
    if out is None:
        out = torch.empty(lead + (F,), dtype=torch.float32, device=bits.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != lead + (F,)
          or not out.is_contiguous() or out.device != bits.device):
        raise ValueError("out must be a contiguous float32 tensor of shape %s on %s" % (lead + (F,), bits.device))
    with torch.cuda.device(bits.device):
        _lib.check(_lib.load().wab_features_unpack(bits.data_ptr(), n, F, out.data_ptr(), _stream(bits)),
                   "wab_features_unpack")
    return out
