"""TOML configuration files (model / dataset), same keys as the reference (``robosat/config.py``, ``config/*.toml``).

Model:   [common] cuda, batch_size, image_size, checkpoint   [opt] epochs, lr, loss
         [augment] zoom, brightness, contrast, saturation, gamma   (extension, optional: robosat_amd/augment.py)
         [opt] boundary_weight, boundary_sigma   (extension, optional: the boundary weight of CrossEntropy / Focal, ``boundary_options`` below)
         [opt] separation_weight, separation_sigma   (extension, optional: the separation weight of CrossEntropy / Focal, ``separation_options`` below)
         [opt] hard_fraction, hard_below   (extension, optional: hard-pixel mining of CrossEntropy / Focal, ``hard_options`` below)
         [opt] relax   (extension, optional: boundary label relaxation of CrossEntropy / Focal, ``relax_options`` below)
         [opt] tversky_alpha, tversky_beta, tversky_gamma, tversky_smooth, tversky_per_image, tversky_classes, tversky_ce
               (extension, optional: the parameters of ``loss = "Tversky"``, ``tversky_options`` below)
         [opt] cldice, cldice_iters, cldice_smooth, cldice_classes
               (extension, optional: the clDice topology term on top of any ``loss``, ``cldice_options`` below)
Dataset: [common] dataset, classes, colors                  [weights] values
         [common] ignore   (extension, optional: the label value of pixels that carry no class, ``ignore_label`` below)
``cuda = true`` means "use the MI355X" (the HIP device shows up as torch's ``cuda``); ``cuda = false`` is rejected by
the tools because this implementation has no CPU compute path.
"""

import tomli

# Class counts the tools accept, stated once.  The reference's model takes any count but its tools are binary
# (predict.py:98 asserts two classes; metrics.py:27-41 counts a 2x2 table): here the kernels behind the losses, the C x C
# confusion matrix and the head take 2..8 classes, and a probability PNG holds one byte per non-background class in at most
# 4 channels (mode P / LA / RGB / RGBA), i.e. up to 5 classes for `rs predict` -> `rs masks`.
MIN_CLASSES, MAX_CLASSES_TRAIN, MAX_CLASSES_PREDICT = 2, 8, 5


def check_num_classes(num_classes, tool):
    """Raises ``ValueError`` when ``tool`` ("train" | "predict" | "serve") cannot handle ``num_classes`` classes."""

    hi = MAX_CLASSES_PREDICT if tool == "predict" else MAX_CLASSES_TRAIN
    if not MIN_CLASSES <= num_classes <= hi:
        raise ValueError("rs {} handles {}..{} classes; the dataset config lists {}".format(tool, MIN_CLASSES, hi, num_classes))


def ignore_label(dataset):
    """The dataset config's optional ``[common] ignore``: the label byte of pixels that carry none of the classes (nodata, unmapped
    ground, "don't know").  ``rs train`` leaves them out of the loss, ``rs weights`` out of the counts and ``rs evaluate`` out of the
    pixel scores.  Returns ``None`` without the key; raises ``ValueError`` unless it is an integer with
    ``len(classes) <= ignore <= 255`` (a label tile holds bytes, and a class index cannot be ignored)."""

    common = dataset["common"]
    if "ignore" not in common:
        return None
    value, num_classes = common["ignore"], len(common["classes"])
    if isinstance(value, bool) or not isinstance(value, int) or not num_classes <= value <= 255:
        raise ValueError("[common] ignore must be an integer in {}..255 (no class index of the {} classes, and a byte), got {}".format(
            num_classes, num_classes, _fmt(value) if isinstance(value, (bool, int, float, str)) else repr(value)))
    return value


BOUNDARY_LOSSES = ("CrossEntropy", "Focal")
BOUNDARY_DEFAULT_SIGMA = 3.0
BOUNDARY_MAX_REACH = 128  # (the radius rs_features_edt takes: include/robosat_hip.h)


def boundary_options(model):
    """The model config's optional ``[opt] boundary_weight`` (w0) and ``[opt] boundary_sigma`` (pixels, 3.0 when only the weight is
    given): the boundary weight ``1 + w0 exp(-d^2 / (2 sigma^2))`` of CrossEntropy and Focal.  Returns ``None`` without the keys, else
    ``(w0, sigma)``; raises ``ValueError("[opt] boundary_...")`` on a value that is no finite number > 0, on ``ceil(3 sigma) > 128``, on
    a sigma without a weight and on a loss that has no per-pixel weight."""

    import math

    opt = model["opt"]
    if "boundary_weight" not in opt:
        if "boundary_sigma" in opt:
            raise ValueError("[opt] boundary_sigma needs [opt] boundary_weight (the weight w0 at a boundary pixel)")
        return None
    values = {}
    for key, default in (("boundary_weight", None), ("boundary_sigma", BOUNDARY_DEFAULT_SIGMA)):
        value = opt.get(key, default)
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not value > 0:
            raise ValueError("[opt] {} must be a finite number > 0, got {}".format(
                key, _fmt(value) if isinstance(value, (bool, int, float, str)) else repr(value)))
        values[key] = float(value)
    reach = int(math.ceil(3.0 * values["boundary_sigma"]))
    if reach > BOUNDARY_MAX_REACH:
        raise ValueError("[opt] boundary_sigma = {} reaches ceil(3 sigma) = {} pixels; at most {}".format(
            _fmt(values["boundary_sigma"]), reach, BOUNDARY_MAX_REACH))
    if opt.get("loss") not in BOUNDARY_LOSSES:
        raise ValueError("[opt] boundary_weight weighs the pixels of {} only; [opt] loss = {} has no per-pixel weight".format(
            " and ".join(BOUNDARY_LOSSES), _fmt(opt.get("loss")) if isinstance(opt.get("loss"), str) else repr(opt.get("loss"))))
    return values["boundary_weight"], values["boundary_sigma"]


SEPARATION_LOSSES = ("CrossEntropy", "Focal")
SEPARATION_DEFAULT_SIGMA = 5.0  # (the U-Net paper's)
SEPARATION_MAX_REACH = 32  # (the reach rs_separation_weight_plane takes: include/robosat_hip.h)


def separation_options(model, dataset=None):
    """The model config's optional ``[opt] separation_weight`` (ws) and ``[opt] separation_sigma`` (pixels, 5.0 when only the weight is
    given): the separation weight ``ws exp(-(d1 + d2)^2 / (2 sigma^2))`` that CrossEntropy and Focal add at a background pixel, d1 and
    d2 its distances to the two nearest objects.  Returns ``None`` without the keys, else ``(ws, sigma)``; raises
    ``ValueError("[opt] separation_...")`` on a value that is no finite number > 0, on ``ceil(3 sigma) > 32``, on a sigma without a
    weight, on a loss that has no per-pixel weight and, where the ``dataset`` config is given, on a dataset with a single class (there
    is no object class: class 0 is the background)."""

    import math

    opt = model["opt"]
    if "separation_weight" not in opt:
        if "separation_sigma" in opt:
            raise ValueError("[opt] separation_sigma needs [opt] separation_weight (the weight ws in a gap of zero width)")
        return None
    values = {}
    for key, default in (("separation_weight", None), ("separation_sigma", SEPARATION_DEFAULT_SIGMA)):
        value = opt.get(key, default)
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not value > 0:
            raise ValueError("[opt] {} must be a finite number > 0, got {}".format(
                key, _fmt(value) if isinstance(value, (bool, int, float, str)) else repr(value)))
        values[key] = float(value)
    reach = int(math.ceil(3.0 * values["separation_sigma"]))
    if reach > SEPARATION_MAX_REACH:
        raise ValueError("[opt] separation_sigma = {} reaches ceil(3 sigma) = {} pixels; at most {}".format(
            _fmt(values["separation_sigma"]), reach, SEPARATION_MAX_REACH))
    if opt.get("loss") not in SEPARATION_LOSSES:
        raise ValueError("[opt] separation_weight weighs the pixels of {} only; [opt] loss = {} has no per-pixel weight".format(
            " and ".join(SEPARATION_LOSSES), _fmt(opt.get("loss")) if isinstance(opt.get("loss"), str) else repr(opt.get("loss"))))
    if dataset is not None and len(dataset["common"]["classes"]) < 2:
        raise ValueError("[opt] separation_weight needs an object class: class 0 is the background and the dataset config lists {} "
                         "class".format(len(dataset["common"]["classes"])))
    return values["separation_weight"], values["separation_sigma"]


HARD_LOSSES = ("CrossEntropy", "Focal")


def hard_options(model):
    """The model config's optional ``[opt] hard_fraction`` (a finite number in (0, 1]) and ``[opt] hard_below`` (a number in (0, 1), needs
    the fraction): hard-pixel mining of CrossEntropy and Focal -- while training, per image only the ``ceil(fraction * valid pixels)``
    pixels of the largest cross-entropy, and every pixel whose true class has a probability below ``hard_below``, count in the loss.
    Returns ``None`` without the keys, else ``(fraction, below | None)``; raises ``ValueError("[opt] hard_...")`` on a bad value, on a
    bound without a fraction and on a loss that has no per-pixel weight."""

    import math

    opt = model["opt"]

    def number(key, ok, what):
        value = opt[key]
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not ok(value):
            raise ValueError("[opt] {} must be {}, got {}".format(
                key, what, _fmt(value) if isinstance(value, (bool, int, float, str)) else repr(value)))
        return float(value)

    if "hard_fraction" not in opt:
        if "hard_below" in opt:
            raise ValueError("[opt] hard_below needs [opt] hard_fraction (the share of an image's pixels that is always kept)")
        return None
    fraction = number("hard_fraction", lambda v: 0 < v <= 1, "a finite number in (0, 1]")
    below = number("hard_below", lambda v: 0 < v < 1, "a number in (0, 1)") if "hard_below" in opt else None
    if opt.get("loss") not in HARD_LOSSES:
        raise ValueError("[opt] hard_fraction mines the pixels of {} only; [opt] loss = {} has no per-pixel weight".format(
            " and ".join(HARD_LOSSES), _fmt(opt.get("loss")) if isinstance(opt.get("loss"), str) else repr(opt.get("loss"))))
    return fraction, below


RELAX_LOSSES = ("CrossEntropy", "Focal")
RELAX_MAX_RADIUS = 16  # (the radius rs_label_set_plane takes: include/robosat_hip.h)


def relax_options(model):
    """The model config's optional ``[opt] relax`` (R, whole pixels): boundary label relaxation of CrossEntropy and Focal -- while
    training, a pixel within R pixels (in x and in y) of other classes is charged for the probability of all of them together, so
    labels that are shifted by up to R pixels cost nothing near an outline.  Returns ``None`` without the key, else R; raises
    ``ValueError("[opt] relax ...")`` unless it is an integer in 1..16, on a loss that has no per-pixel term and beside
    ``[opt] hard_fraction`` (mining would have to rank the pixels by their relaxed loss, which is not implemented)."""

    opt = model["opt"]
    if "relax" not in opt:
        return None
    value = opt["relax"]
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= RELAX_MAX_RADIUS:
        raise ValueError("[opt] relax must be an integer radius in 1..{} pixels, got {}".format(
            RELAX_MAX_RADIUS, _fmt(value) if isinstance(value, (bool, int, float, str)) else repr(value)))
    if opt.get("loss") not in RELAX_LOSSES:
        raise ValueError("[opt] relax relaxes the pixel terms of {} only; [opt] loss = {} has none".format(
            " and ".join(RELAX_LOSSES), _fmt(opt.get("loss")) if isinstance(opt.get("loss"), str) else repr(opt.get("loss"))))
    if "hard_fraction" in opt:
        raise ValueError("[opt] relax cannot stand beside [opt] hard_fraction: mining ranks the pixels by their strict cross-entropy, "
                         "which is largest on the band that relaxation forgives; ranking by the relaxed loss is not implemented")
    return value


TVERSKY_LOSS = "Tversky"
TVERSKY_KEYS = ("tversky_alpha", "tversky_beta", "tversky_gamma", "tversky_smooth", "tversky_per_image", "tversky_classes", "tversky_ce")


def tversky_options(model):
    """The model config's optional ``[opt] tversky_alpha`` / ``tversky_beta`` (the weights of false positives / false negatives, 0.5
    each = Dice; >= 0 and not both 0), ``tversky_gamma`` (> 0, 1.0; below 1 = focal Tversky), ``tversky_smooth`` (>= 0, 1.0),
    ``tversky_per_image`` (true), ``tversky_classes`` ("present" | "all", "present") and ``tversky_ce`` (>= 0, 0.0: the factor of the
    fused cross-entropy term) of ``[opt] loss = "Tversky"``.  Returns ``None`` for another loss, else the keyword arguments of
    ``TverskyLoss2d``; raises ``ValueError("[opt] tversky_...")`` on a bad value, and on any of the keys beside another loss."""

    import math

    opt = model["opt"]
    given = [key for key in TVERSKY_KEYS if key in opt]
    if opt.get("loss") != TVERSKY_LOSS:
        if given:
            raise ValueError("[opt] {} belongs to [opt] loss = {}; [opt] loss = {} does not read it".format(
                given[0], _fmt(TVERSKY_LOSS), _fmt(opt.get("loss")) if isinstance(opt.get("loss"), str) else repr(opt.get("loss"))))
        return None

    def shown(value):
        return _fmt(value) if isinstance(value, (bool, int, float, str)) else repr(value)

    def number(key, default, ok, what):
        value = opt.get(key, default)
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not ok(value):
            raise ValueError("[opt] {} must be {}, got {}".format(key, what, shown(value)))
        return float(value)

    alpha = number("tversky_alpha", 0.5, lambda v: v >= 0, "a finite number >= 0")
    beta = number("tversky_beta", 0.5, lambda v: v >= 0, "a finite number >= 0")
    if alpha == 0 and beta == 0:
        raise ValueError("[opt] tversky_alpha and tversky_beta must not both be 0 (the index would ignore every error)")
    gamma = number("tversky_gamma", 1.0, lambda v: v > 0, "a finite number > 0")
    smooth = number("tversky_smooth", 1.0, lambda v: v >= 0, "a finite number >= 0")
    ce = number("tversky_ce", 0.0, lambda v: v >= 0, "a finite number >= 0")
    per_image = opt.get("tversky_per_image", True)
    if not isinstance(per_image, bool):
        raise ValueError("[opt] tversky_per_image must be true or false, got {}".format(shown(per_image)))
    classes = opt.get("tversky_classes", "present")
    if classes not in ("present", "all"):
        raise ValueError("[opt] tversky_classes must be \"present\" or \"all\", got {}".format(shown(classes)))
    return {"alpha": alpha, "beta": beta, "gamma": gamma, "smooth": smooth, "per_image": per_image, "classes": classes, "ce": ce}


CLDICE_KEYS = ("cldice_iters", "cldice_smooth", "cldice_classes")
CLDICE_DEFAULT_ITERS = 10  # (the paper's code takes 3 for thin vessels; a road is wider)
CLDICE_MAX_ITERS = 64  # (what rs_soft_skeleton_fwd takes: include/robosat_hip.h)


def cldice_options(model, dataset):
    """The model config's optional ``[opt] cldice`` (a, ``0 < a < 1``: the loss becomes ``(1 - a) x [opt] loss + a x clDice``) with
    ``cldice_iters`` (an integer in 1..64, 10: the iterations of the soft skeleton, at least half the widest road in pixels -- a
    structure wider than ``2 x iters`` pixels is not thinned to its centre line), ``cldice_smooth`` (>= 0, 1.0) and ``cldice_classes``
    (a list of non-background class names of the dataset config, all of them by default).  Returns ``None`` without the keys, else the
    keyword arguments of ``ClDiceLoss2d`` after ``base`` (``classes`` as indices, ``None`` for all); raises
    ``ValueError("[opt] cldice...")`` on a bad value, on a ``cldice_*`` key without ``cldice`` and on an unknown class name."""

    import math

    opt = model["opt"]

    def shown(value):
        return _fmt(value) if isinstance(value, (bool, int, float, str)) else repr(value)

    if "cldice" not in opt:
        for key in CLDICE_KEYS:
            if key in opt:
                raise ValueError("[opt] {} needs [opt] cldice (the weight a of the clDice term, 0 < a < 1)".format(key))
        return None
    a = opt["cldice"]
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a) or not 0 < a < 1:
        raise ValueError("[opt] cldice must be a number with 0 < a < 1, got {}".format(shown(a)))
    iters = opt.get("cldice_iters", CLDICE_DEFAULT_ITERS)
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= CLDICE_MAX_ITERS:
        raise ValueError("[opt] cldice_iters must be an integer in 1..{}, got {}".format(CLDICE_MAX_ITERS, shown(iters)))
    smooth = opt.get("cldice_smooth", 1.0)
    if isinstance(smooth, bool) or not isinstance(smooth, (int, float)) or not math.isfinite(smooth) or smooth < 0:
        raise ValueError("[opt] cldice_smooth must be a finite number >= 0, got {}".format(shown(smooth)))
    names = list(dataset["common"]["classes"])
    if len(names) < 2:
        raise ValueError("[opt] cldice needs a non-background class: class 0 is the background and the dataset config lists {} "
                         "class".format(len(names)))
    classes = None
    if "cldice_classes" in opt:
        picked = opt["cldice_classes"]
        if not isinstance(picked, list) or not picked or not all(isinstance(name, str) for name in picked):
            raise ValueError("[opt] cldice_classes must be a non-empty list of class names, got {}".format(shown(picked)))
        if len(set(picked)) != len(picked):
            raise ValueError("[opt] cldice_classes names a class twice: {}".format(shown(picked)))
        for name in picked:
            if name not in names[1:]:
                raise ValueError("[opt] cldice_classes: {} is no non-background class of the dataset config ({})".format(
                    _fmt(name), ", ".join(_fmt(known) for known in names[1:])))
        classes = tuple(sorted(names.index(name, 1) for name in picked))
    return {"weight": float(a), "iters": iters, "smooth": float(smooth), "classes": classes}


OPTIMIZER_KEYS = ("weight_decay", "schedule", "schedule_power", "warmup_steps", "lr_min", "clip_norm", "ema")
OPTIMIZER_SCHEDULES = ("constant", "poly", "cosine")


def optimizer_options(model):
    """The model config's optional ``[opt] weight_decay`` (>= 0), ``schedule`` ("constant" | "poly" | "cosine") with ``schedule_power``
    (> 0, 0.9; poly's exponent), ``warmup_steps`` (an integer >= 0, 0) and ``lr_min`` (>= 0 and <= lr, 0), ``clip_norm`` (> 0) and
    ``ema`` (in (0, 1)): any one of them selects the native optimiser (``robosat_amd.optim.AdamW``).  Returns ``None`` without the
    keys -- the reference's ``Adam(lr)`` --, else ``{"weight_decay", "schedule" | None, "schedule_power", "warmup_steps", "lr_min",
    "clip_norm" | None, "ema" | None}``; raises ``ValueError("[opt] ...")`` on a bad value, and on ``schedule_power``, ``warmup_steps``
    or ``lr_min`` without ``schedule``."""

    import math

    opt = model["opt"]
    if not any(key in opt for key in OPTIMIZER_KEYS):
        return None

    def shown(value):
        return _fmt(value) if isinstance(value, (bool, int, float, str)) else repr(value)

    def number(key, default, ok, what):
        value = opt.get(key, default)
        if value is None:
            return None
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not ok(value):
            raise ValueError("[opt] {} must be {}, got {}".format(key, what, shown(value)))
        return float(value)

    schedule = opt.get("schedule")
    if schedule is None:
        for key in ("schedule_power", "warmup_steps", "lr_min"):
            if key in opt:
                raise ValueError("[opt] {} needs [opt] schedule (one of {})".format(
                    key, ", ".join('"{}"'.format(s) for s in OPTIMIZER_SCHEDULES)))
    elif schedule not in OPTIMIZER_SCHEDULES:
        raise ValueError("[opt] schedule must be one of {}, got {}".format(
            ", ".join('"{}"'.format(s) for s in OPTIMIZER_SCHEDULES), shown(schedule)))
    lr = opt.get("lr")
    if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not math.isfinite(lr) or not lr > 0:
        raise ValueError("[opt] lr must be a finite number > 0 for the native optimiser, got {}".format(shown(lr)))
    warmup = opt.get("warmup_steps", 0)
    if isinstance(warmup, bool) or not isinstance(warmup, int) or warmup < 0:
        raise ValueError("[opt] warmup_steps must be an integer >= 0, got {}".format(shown(warmup)))
    return {
        "weight_decay": number("weight_decay", 0.0, lambda v: v >= 0, "a finite number >= 0"),
        "schedule": schedule,
        "schedule_power": number("schedule_power", 0.9, lambda v: v > 0, "a finite number > 0"),
        "warmup_steps": warmup,
        "lr_min": number("lr_min", 0.0, lambda v: 0 <= v <= lr, "a finite number in [0, lr]"),
        "clip_norm": number("clip_norm", None, lambda v: v > 0, "a finite number > 0"),
        "ema": number("ema", None, lambda v: 0 < v < 1, "a number in (0, 1)"),
    }


def load_config(path):
    """Parses the TOML file at ``path`` into a dictionary."""

    with open(path, "rb") as fp:
        return tomli.load(fp)


def _fmt(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, (int, float)):
        return repr(v)
    if isinstance(v, str):
        return "'{}'".format(v) if "'" not in v else '"{}"'.format(v.replace("\\", "\\\\").replace('"', '\\"'))
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(_fmt(x) for x in v) + "]"
    raise TypeError("unsupported TOML value: {!r}".format(v))


def save_config(attrs, path):
    """Writes a two-level configuration dictionary (``{table: {key: scalar | list}}``) as TOML."""

    with open(path, "w") as fp:
        for table, entries in attrs.items():
            fp.write("[{}]\n".format(table))
            for key, value in entries.items():
                fp.write("  {} = {}\n".format(key, _fmt(value)))
            fp.write("\n")
