"""Circular-padding restatement of the oracle's functional UNet (oracle/pidm_oracle.py: unet_forward), for
Unet3D(padding_mode='circular') (reference: src/unet_model.py:161-199, 224-229, 452-455, 480-511).  TEST INFRASTRUCTURE.

The oracle module itself is not touched: while `unet_forward` runs, its `F` is replaced by a proxy whose conv2d / conv_transpose2d
wrap around -
  * conv2d with padding p > 0: F.pad(x, p on every side, mode='circular') followed by the unpadded convolution (what
    nn.Conv3d(padding_mode='circular') does);
  * conv_transpose2d 4x4 / stride 2 / padding 1: the reference's CircularUpsample - circular pad by 2, transposed convolution with
    padding 5;
  * kernel-size-1 convolutions (padding 0) and the conditioning branch's emb_conv.2, which the reference builds with
    padding_mode='zeros' (:524), pass through.
The reference keeps the upsampling weights in a sub-module: `ups.i.3.conv_transpose.{weight,bias}`; the parameter dictionary is
given the oracle's `ups.i.3.{weight,bias}` names as aliases of the SAME tensors, so gradients land in the caller's tensors.
tests/test_unet_circular.py holds this restatement to tests/golden/g28_unet_circular.npz (the reference's own results) before it
uses it as a yardstick."""
import contextlib

import torch
import torch.nn.functional as TF

from oracle import pidm_oracle as O


def circular_conv2d(x, w, b=None, stride=1, padding=0):
    if padding:
        x = TF.pad(x, (padding,) * 4, mode="circular")
    return TF.conv2d(x, w, b, stride=stride)


def circular_conv_transpose2d(x, w, b=None):
    """out[y] = sum_j x[j mod H] w[y + 1 - 2j]: the zero-mode ConvTranspose 4x4 / s2 / p1 with wrapped reads."""
    return TF.conv_transpose2d(TF.pad(x, (2, 2, 2, 2), mode="circular"), w, b, stride=2, padding=5)


class _CircularF:
    def __init__(self, zero_padded):
        self._zero = [id(t) for t in zero_padded]

    def __getattr__(self, name):
        return getattr(TF, name)

    def conv2d(self, x, w, b=None, stride=1, padding=0):
        if padding == 0 or id(w) in self._zero:
            return TF.conv2d(x, w, b, stride=stride, padding=padding)
        return circular_conv2d(x, w, b, stride, padding)

    def conv_transpose2d(self, x, w, b=None, stride=1, padding=0):
        assert stride == 2 and padding == 1 and w.shape[-1] == 4, "the oracle's only transposed convolution is 4x4 / s2 / p1"
        return circular_conv_transpose2d(x, w, b)


@contextlib.contextmanager
def circular_functional(zero_padded=()):
    saved = O.F
    O.F = _CircularF(zero_padded)
    try:
        yield
    finally:
        O.F = saved


def unet_forward_circular(p, x, t, cfg, cond=None):
    """`p`: parameters under the circular model's state_dict names."""
    q = dict(p)
    for k, v in p.items():
        if ".3.conv_transpose." in k:
            q[k.replace(".3.conv_transpose.", ".3.")] = v
    with circular_functional([p["emb_conv.2.weight"]] if "emb_conv.2.weight" in p else ()):
        return O.unet_forward(q, x, t, cfg, cond=cond)
