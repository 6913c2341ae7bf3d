"""The fixed cases behind tests/golden/loss_bits.json: every entry point of csrc/loss.hip and csrc/lovasz.hip on inputs made from
integer arithmetic alone (no library random generator: the same bytes anywhere), and the SHA-256 of each output's raw bytes.
Shared by scripts/record_loss_bits.py, which writes the golden file on the MI355X, and tests/test_gpu_loss_bits.py, which
recomputes the digests and compares them.  The kernels are deterministic (fixed reduction trees, integer atomics only), so a
digest pins a build's bits.

Shapes (N, C, H, W): the smallest that reach every path of these kernels.
    (2, 2, 5, 7)      P below one block; HW % 4 != 0: the scalar lovasz_keys and VEC = 1 paths
    (3, 3, 16, 16)    HW % 4 == 0: the keys4 and VEC = 4 paths
    (8, 2, 24, 24)    N % 8 == 0: xcd_affine in the apply kernels
    (16, 2, 8, 8)     sc_affine in the sort
    (2, 8, 9, 9)      C = kMaxC
    (1, 1, 4, 4)      C = 1: NLL, mIoU and hinge only
    (2, 2, 384, 384)  NLL and mIoU only: more than kLossBlocks * 256 pixels and more than kMiouBlocks * 256 per image, so both
                      grid-stride loops take a second trip
Ignore patterns: none, about 30 % scattered, one whole image, everything (the last for the `_ig` / `_pw` entries only)."""

import hashlib

import numpy as np

SHAPES = [(2, 2, 5, 7), (3, 3, 16, 16), (8, 2, 24, 24), (16, 2, 8, 8), (2, 8, 9, 9), (1, 1, 4, 4), (2, 2, 384, 384)]
NLL_MIOU_ONLY = {(2, 2, 384, 384)}
IGNORE = 255
PATTERNS = ("none", "scattered", "image", "all")
GAMMA = 2.0
W0, SIGMA = 4.0, 1.5
_MASK = (1 << 64) - 1


def shape_key(shape):
    return "x".join(str(d) for d in shape)


def _hash(count, salt):
    """uint64 [count]: a 64-bit mix (splitmix64's finaliser) of index and salt, in wrapping uint64 arithmetic."""

    with np.errstate(over="ignore"):
        h = np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((salt * 0xD1B54A32D192ED03 + 1) & _MASK)
        h ^= h >> np.uint64(30)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(27)
        h *= np.uint64(0x94D049BB133111EB)
        h ^= h >> np.uint64(31)
    return h


def logits(shape):
    """float32 [N, C, H, W] in [-4, 4): 24 hash bits over 2^21, exact in float32."""

    n, c, h, w = shape
    bits = (_hash(n * c * h * w, 1) >> np.uint64(40)).astype(np.int64)
    return ((bits - (1 << 23)).astype(np.float32) / np.float32(1 << 21)).reshape(shape)


def labels(shape, pattern):
    """int64 [N, H, W]: 3 x 4 blocks of one class (label boundaries for the weight plane) with one pixel in eight re-drawn, then
    the ignore pattern on top."""

    n, c, h, w = shape
    nn, yy, xx = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    hv = _hash(n * h * w, 2).reshape(n, h, w)
    t = (nn + yy // 3 + xx // 4) % c
    t = np.where((hv & np.uint64(7)) == 0, ((hv >> np.uint64(8)) % np.uint64(c)).astype(np.int64), t).astype(np.int64)
    if pattern == "scattered":
        t[(_hash(n * h * w, 3).reshape(n, h, w) >> np.uint64(16)) % np.uint64(10) < 3] = IGNORE
    elif pattern == "image":
        t[n - 1] = IGNORE
    elif pattern == "all":
        t[:] = IGNORE
    else:
        assert pattern == "none", pattern
    return t


def class_weight(c):
    return (1.0 + 0.5 * np.arange(c)).astype(np.float32)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_shape(shape, device="cuda:0"):
    """case id -> {output name -> sha256} for every entry point that takes ``shape``, through robosat_amd.ops."""

    import torch

    from robosat_amd import ops

    n, c, h, w = shape
    x = torch.from_numpy(logits(shape)).to(device)
    tgt = {p: torch.from_numpy(labels(shape, p)).to(device) for p in PATTERNS}
    gout = torch.tensor(0.75, device=device)
    out = {}

    plane = {}
    for p in PATTERNS:
        ig = None if p == "none" else IGNORE
        plane[p] = ops.boundary_weight_plane(tgt[p], W0, SIGMA, ignore=ig, classes=c)
        out["boundary_weight_plane/{}".format(p)] = {"plane": digest(plane[p])}

    # (entry, labels' pattern, ignore, pixel weight): plain on the clean labels, `_ig` and `_pw` on all four patterns; `_pw` with no
    # pixel ignored passes ignore = None, the -1 of its C ABI
    variants = [("plain", "none", None, None)]
    variants += [("ig", p, IGNORE, None) for p in PATTERNS]
    variants += [("pw", p, None if p == "none" else IGNORE, plane[p]) for p in PATTERNS]

    for wname, cw, go in (("w-none", None, None), ("w-given", torch.from_numpy(class_weight(c)).to(device), gout)):
        for entry, p, ig, pw in variants:
            for mname, mode in (("CrossEntropy", ops.NLL_CROSS_ENTROPY), ("Focal", ops.NLL_FOCAL)):
                loss, stats = ops.nll_loss_fwd(x, tgt[p], cw, mode, GAMMA, ignore=ig, pixel_weight=pw)
                kept = stats.clone()
                grad = ops.nll_loss_bwd(x, tgt[p], cw, stats, go, mode, GAMMA, ignore=ig, pixel_weight=pw)
                out["nll_{}/{}/{}/{}".format(entry, mname, wname, p)] = {"loss": digest(loss), "stats": digest(kept), "grad": digest(grad)}
            if entry == "pw":
                continue
            loss, stats = ops.miou_loss_fwd(x, tgt[p], cw, ignore=ig)
            kept = stats.clone()
            grad = ops.miou_loss_bwd(x, tgt[p], cw, stats, go, ignore=ig)
            out["miou_{}/{}/{}".format(entry, wname, p)] = {"loss": digest(loss), "stats": digest(kept), "grad": digest(grad)}

    counts = torch.zeros(4, device=device, dtype=torch.int64)
    out["confusion_counts"] = {"counts": digest(ops.confusion_counts(x, tgt["none"], counts))}
    out["scale_by_scalar"] = {"out": digest(ops.scale_by_scalar(x, gout.reshape(1)))}
    if shape in NLL_MIOU_ONLY:
        return out

    for entry, p, ig, pw in variants:
        if entry == "pw":
            continue
        loss, grad = ops.lovasz_fwd(x, tgt[p], want_grad=True, ignore=ig)
        out["lovasz_{}/{}".format(entry, p)] = {"loss": digest(loss), "grad": digest(grad)}
        loss, _ = ops.lovasz_fwd(x, tgt[p], want_grad=False, ignore=ig)
        out["lovasz_{}/{}/no-grad".format(entry, p)] = {"loss": digest(loss)}
        if c < 2:
            continue
        for per_image in (True, False):
            for classes in ("present", "all"):
                loss, grad, probs = ops.lovasz_softmax_fwd(x, tgt[p], per_image=per_image, classes=classes, want_grad=True,
                                                           want_probs=True, ignore=ig)
                out["lovasz_softmax_{}/{}/{}/{}".format(entry, "per-image" if per_image else "batch", classes, p)] = {
                    "loss": digest(loss), "grad": digest(grad), "probs": digest(probs)}
    return out
