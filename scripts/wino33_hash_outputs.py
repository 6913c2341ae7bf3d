"""sha256 of the outputs of every conv_wino33_f32 instantiation (plain, + scale / shift / ReLU, statistics, data gradient with float /
bit / no mask, the fused head at 1 .. 8 classes in its four output kinds) on the shapes of tests/test_gpu_wino33_items.py and a few
of the benchmark's.  The library is whatever ROBOSAT_HIP_LIB names, else the tree's: run from the repository root once per library
and diff the two listings (profiles/wino33_items/hashes.txt)."""
import hashlib
import sys

import torch

sys.path.insert(0, ".")
from robosat_amd import ops  # noqa: E402

DEV = "cuda:0"


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def h(name, t):
    if t is None:
        print(name, "None")
        return
    torch.cuda.synchronize()
    print(name, hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:24], tuple(t.shape))


PLAIN = [(6, 64, 64, 32, 256), (3, 16, 16, 32, 48), (2, 17, 31, 48, 64), (2, 40, 24, 48, 64), (5, 64, 48, 15 + 17, 96), (16, 128, 128, 64, 64)]
for n, hh, w, cin, cout in PLAIN:
    g = gen(1)
    x = torch.randn(n, hh, w, cin, device=DEV, generator=g)
    wk = torch.randn(cout, 3, 3, cin, device=DEV, generator=g) * (2.0 / (9 * cin)) ** 0.5
    sc, sh = torch.rand(cout, device=DEV, generator=g) + 0.5, torch.randn(cout, device=DEV, generator=g) * 0.3
    u = ops.pack_wino33_weight(wk)
    tag = "{}x{}x{}x{}->{}".format(n, hh, w, cin, cout)
    h("plain " + tag, ops.conv2d_wino33(x, u))
    h("plain+bn+relu " + tag, ops.conv2d_wino33(x, u, scale=sc, shift=sh, relu=True))
    o, p = ops.conv2d_wino33_bnstats(x, u)
    h("stats.out " + tag, o)
    h("stats.part " + tag, p)

for n, hh, w, cin, cout in [(2, 17, 31, 64, 48), (6, 64, 64, 32, 64), (2, 40, 24, 32, 32)]:
    g = gen(2)
    y1 = torch.randn(n, hh, w, cin, device=DEV, generator=g)
    wk = torch.randn(cout, 3, 3, cin, device=DEV, generator=g) * (2.0 / (9 * cin)) ** 0.5
    dy = torch.randn(n, hh, w, cout, device=DEV, generator=g)
    mean, var = y1.mean((0, 1, 2)), y1.var((0, 1, 2), unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    z, bits = ops.bn_apply(y1, invstd, -mean * invstd, relu=True, want_bits=True)
    u = ops.pack_wino33_weight(ops.pack_dgrad_weight(wk))
    tag = "{}x{}x{}x{}<-{}".format(n, hh, w, cin, cout)
    for name, kw in (("float", dict(relu_mask=z)), ("bits", dict(relu_mask_bits=bits)), ("nomask", {})):
        gq, pq = ops.conv2d_wino33_dgrad(dy, u, bn=(y1, mean, invstd), **kw)
        h("bwd {} g {}".format(name, tag), gq)
        h("bwd {} part {}".format(name, tag), pq)
        gq, _ = ops.conv2d_wino33_dgrad(dy, u, **kw)
        h("bwd {} g nobn {}".format(name, tag), gq)

for n, hh, w in [(2, 32, 48), (2, 17, 31), (5, 128, 128), (37, 16, 16)]:
    for classes in (1, 2, 3, 4, 5, 6, 7, 8):
        if hh == 128 and classes not in (2, 4, 8):
            continue
        g = gen(3 + classes)
        x = torch.randn(n, hh, w, 32, device=DEV, generator=g)
        wk = torch.randn(32, 3, 3, 32, device=DEV, generator=g) * (2.0 / (9 * 32)) ** 0.5
        fw = torch.randn(classes, 32, device=DEV, generator=g) * 0.5
        fb = torch.randn(classes, device=DEV, generator=g) * 0.2
        u = ops.pack_wino33_weight(wk)
        tag = "{}x{}x{} C={}".format(n, hh, w, classes)
        h("head logits " + tag, ops.conv2d_wino33_head(x, u, fw, fb, "logits"))
        h("head softmax " + tag, ops.conv2d_wino33_head(x, u, fw, fb, "softmax"))
        h("head logits nobias " + tag, ops.conv2d_wino33_head(x, u, fw, None, "logits"))
        if classes >= 2:
            h("head argmax " + tag, ops.conv2d_wino33_head(x, u, fw, fb, "argmax"))
            h("head quantize ov0 " + tag, ops.conv2d_wino33_head(x, u, fw, fb, "quantize", overlap=0))
            h("head quantize ov3 " + tag, ops.conv2d_wino33_head(x, u, fw, fb, "quantize", overlap=3))
