"""Writes tests/golden/g28_unet_circular.npz from the reference's own `Unet3D(padding_mode='circular')` (src/unet_model.py of the
checkout given by --reference).  CPU only; runs where the reference checkout exists.

    python tools/make_golden_unet_circular.py --reference /path/to/PhysicsInformedDiffusionModels

Parameters are formula-filled from their state_dict names (oracle/pidm_oracle.fill_state_dict), so nothing but seeded inputs and
the reference's results is stored.  Per case <c>:

  <c>/x [B, C, P, P], <c>/t, <c>/w (cotangent), <c>/cond (the conditioned case), <c>/out = model(x, t)
  <c>/grad_names, <c>/grad_norms     float64 norms of d sum(w * out) / d parameter, every parameter that has a gradient
  <c>/grad/<name>                    the full gradient of the probe tensors
  keys                               state_dict keys of the default circular model, in order (317)

Cases: dim 8 at 16x16 with the default four levels (bottom level 2x2), B = 3; dim 8 at 8x8 with dim_mults (1, 2), B = 2; dim 32 at
32x32 with dim_mults (1, 2, 4), B = 1; the first case again with a conditioning field (emb_conv.2 stays zero-padded).
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# name -> (constructor arguments, image size, batch, conditioned)
CASES = {
    "d8_p16": (dict(dim=8), 16, 3, False),
    "d8_p8_l2": (dict(dim=8, dim_mults=(1, 2)), 8, 2, False),
    "d32_p32_l3": (dict(dim=32, dim_mults=(1, 2, 4)), 32, 1, False),
    "d8_p16_cond": (dict(dim=8), 16, 3, True),
}
PROBES = ("init_conv.weight", "downs.0.0.block1.proj.weight", "downs.0.3.weight", "ups.0.3.conv_transpose.weight",
          "downs.0.2.fn.fn.to_qkv.weight")


def load_reference(path):
    path = os.path.abspath(path)
    sys.path.insert(0, os.path.join(REPO, "oracle", "shims"))   # einops_exts, rotary_embedding_torch: import-only stand-ins
    for name in [m for m in sys.modules if m == "src" or m.startswith("src.")]:
        del sys.modules[name]
    # `src` must be the reference's directory (it has no __init__.py; this repository's own `src` package would win on sys.path)
    pkg = types.ModuleType("src")
    pkg.__path__ = [os.path.join(path, "src")]
    sys.modules["src"] = pkg
    import src.unet_model as um
    assert os.path.abspath(um.__file__).startswith(path + os.sep), (um.__file__, path)
    return um


def load_oracle():
    spec = importlib.util.spec_from_file_location("pidm_oracle", os.path.join(REPO, "oracle", "pidm_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "g28_unet_circular.npz"))
    args = ap.parse_args()
    um = load_reference(args.reference)
    O = load_oracle()
    torch.set_num_threads(8)
    d = {}
    for i, (tag, (kw, P, B, conditioned)) in enumerate(CASES.items()):
        torch.manual_seed(0)
        m = um.Unet3D(channels=2, padding_mode="circular", **kw)
        m.load_state_dict(O.fill_state_dict(m.state_dict()))
        if i == 0:
            d["keys"] = np.array(list(m.state_dict().keys()))
        x = seeded((B, 2, P, P), 2801 + i)
        t = torch.tensor([3, 47, 99][:B], dtype=torch.long)
        x_bxyc = x.permute(0, 2, 3, 1).reshape(B, P * P, 2)
        cond = seeded((B, P * P, 2), 2851 + i) if conditioned else None
        out = m(x_bxyc, t, cond=cond, null_cond_prob=0.) if conditioned else m(x_bxyc, t)
        w = seeded(tuple(out.shape), 2901 + i)
        (out * w).sum().backward()
        d[tag + "/x"], d[tag + "/t"], d[tag + "/w"], d[tag + "/out"] = x.numpy(), t.numpy(), w.numpy(), out.detach().numpy()
        if conditioned:
            d[tag + "/cond"] = cond.numpy()
        named = dict(m.named_parameters())
        names = [k for k, p in named.items() if p.grad is not None]
        d[tag + "/grad_names"] = np.array(names)
        d[tag + "/grad_norms"] = np.array([named[k].grad.double().norm().item() for k in names])
        for k in PROBES:
            d[tag + "/grad/" + k] = named[k].grad.numpy()
        print(tag, "out", tuple(out.shape), "gradients", len(names))
    np.savez_compressed(args.out, **d)
    print(args.out, os.path.getsize(args.out), "bytes")
    assert os.path.getsize(args.out) < (1 << 20)


if __name__ == "__main__":
    main()
