"""sha256 of the outputs of every conv_wino_f32 instantiation: the forward on one and two sources, ReLU on and off, the C1 -> C2 switch on
the first, a middle and the last chunk, nk = 2, ragged patches, blocks that walk 1, 2 and 3+ items, the p4 blocks; the data gradient with a
float mask and none (the kernel takes no bit mask), with and without the split at `csplit`, on both of its block shapes.  The library is
whatever ROBOSAT_HIP_LIB names, else the tree's: run from the repository root once per library and diff the two listings
(profiles/wino_items/hashes.txt)."""
import hashlib
import sys

import torch

sys.path.insert(0, ".")
from robosat_amd import ops  # noqa: E402

DEV = "cuda:0"


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def h(name, t):
    torch.cuda.synchronize()
    print(name, hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:24], tuple(t.shape))


# (n, h, w, c1, c2, cout)
FWD = [
    (2, 16, 16, 16, 16, 64),     # 64 x 64 block, nk = 2, one item per block
    (3, 18, 22, 32, 0, 64),      # one source, ragged patches
    (2, 16, 16, 16, 48, 64),     # the switch on the first chunk boundary
    (2, 16, 16, 32, 48, 64),     # ... on a middle one
    (2, 16, 30, 48, 16, 32),     # ... on the last one; 128 x 32 block
    (3, 18, 22, 32, 0, 32),      # 128 x 32, odd sub-block count: a dead second sub-block
    (5, 16, 16, 16, 16, 32),     # 128 x 32, sub-blocks of one item in two images
    (100, 16, 16, 32, 0, 64),    # 64 x 64: 400 items, one or two per block
    (200, 16, 16, 32, 0, 64),    # 800 items: three or four per block
    (8, 64, 60, 16, 16, 128),    # 128 x 64 block, ragged last patch row
    (16, 64, 64, 16, 16, 64),    # 128 x 64: two items per block
    (16, 64, 64, 32, 0, 128),    # 128 x 64: four items per block
    (4, 64, 64, 32, 0, 32),      # 128 x 32: several items per block
    (3, 8, 12, 32, 0, 64),       # p4, 64 x 64
    (3, 10, 14, 16, 16, 32),     # p4, 128 x 32
    (300, 8, 8, 32, 0, 64),      # p4: one or two items per block
]
for n, hh, w, c1, c2, cout in FWD:
    g = gen(1)
    a = torch.randn(n, hh, w, c1, device=DEV, generator=g)
    b = torch.randn(n, hh, w, c2, device=DEV, generator=g) if c2 else None
    wk = torch.randn(cout, 3, 3, c1 + c2, device=DEV, generator=g) * (2.0 / (9 * (c1 + c2))) ** 0.5
    assert ops.wino_ok(a, b, cout, force=True)
    u = ops.pack_wino_phase_weight(ops.pack_phase_weight(wk))
    tag = "{}x{}x{}x{}+{}->{}".format(n, hh, w, c1, c2, cout)
    h("fwd " + tag, ops.conv2d_phase_wino(a, u, src2=b, relu=False))
    h("fwd+relu " + tag, ops.conv2d_phase_wino(a, u, src2=b, relu=True))

# (n, c1, c2, cout, hs): the FORWARD layer's channels; dz has cout channels at 2 hs
DG = [(2, 32, 32, 64, 16), (3, 64, 0, 32, 18), (2, 64, 64, 32, 16), (70, 64, 64, 32, 16), (16, 128, 128, 32, 64), (16, 64, 64, 32, 128)]
for n, c1, c2, cout, hs in DG:
    assert ops.wino_dgrad_ok(n, hs, hs, c1, c2, cout)
    g = gen(2)
    wk = torch.randn(cout, 3, 3, c1 + c2, device=DEV, generator=g) * 0.05
    dz = torch.randn(n, 2 * hs, 2 * hs, cout, device=DEV, generator=g)
    mask = torch.randn(n, hs, hs, c1 + c2, device=DEV, generator=g)
    u = ops.pack_wino_dgrad_weight(ops.pack_dgrad_phase_weight(wk))
    tag = "{}x{}x{}x{}<-{}+{}".format(n, hs, hs, cout, c1, c2)
    h("dg nomask " + tag, ops.conv2d_dgrad_phase_wino(dz, u, c1, c2)[0])
    h("dg mask " + tag, ops.conv2d_dgrad_phase_wino(dz, u, c1, c2, mask1=mask)[0])
    if c2 and c1 % 64 == 0:
        m1, m2 = mask[..., :c1].contiguous(), mask[..., c1:].contiguous()
        for name, kw in (("split nomask", {}), ("split mask", dict(mask1=m1, mask2=m2)), ("split mask2", dict(mask2=m2))):
            d1, d2 = ops.conv2d_dgrad_phase_wino(dz, u, c1, c2, split=True, **kw)
            h("dg {} d1 {}".format(name, tag), d1)
            h("dg {} d2 {}".format(name, tag), d2)
