"""``rs predict --tta`` and ``rs serve``'s ``Predictor(..., tta=)`` on the MI355X: the files and masks equal the library's
TTA calls, ``--tta none`` writes what a plain run writes, and a two-rank run forwards the flag to its ranks."""

import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import synth
from oracle import robosat_ref as R, seeded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TILE, OVERLAP = 256, 32


def _net(classes, seed):
    from robosat_amd.unet import UNet

    net = UNet(classes, pretrained=False)
    net.load_state_dict(seeded.seeded_state_dict(R.UNetRef(classes).state_dict(), seed))
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("tta_cli"))
    ds_root = synth.make_dataset(os.path.join(tmp, "ds"), n_train=1, n_val=3, size=TILE, seed=5)
    model_toml, ds_toml = synth.write_configs(tmp, ds_root, os.path.join(tmp, "pth"), image_size=TILE)
    net = _net(2, 31)
    ck = os.path.join(tmp, "ck.pth")
    torch.save({"epoch": 1, "state_dict": {"module." + k: v for k, v in net.state_dict().items()}}, ck)
    return {"tmp": tmp, "tiles": os.path.join(ds_root, "validation", "images"), "model": model_toml, "dataset": ds_toml, "ck": ck,
            "net": net}


def _files(probs):
    files = sorted(os.path.relpath(os.path.join(d, f), probs) for d, _, fs in os.walk(probs) for f in fs)
    return {f: np.array(Image.open(os.path.join(probs, f))) for f in files}


def _predict_in_process(s, out, tta=None):
    from robosat_amd.tools import predict

    ns = argparse.Namespace(batch_size=2, checkpoint=s["ck"], overlap=OVERLAP, tile_size=TILE, workers=0, tiles=s["tiles"], probs=out,
                            model=s["model"], dataset=s["dataset"], extra_tiles=[])
    if tta is not None:
        ns.tta = tta
    predict.main(ns)
    return _files(out)


def _rs(args, env_extra, cwd):
    env = dict(os.environ)
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=cwd, capture_output=True, text=True,
                          timeout=900)


def test_predict_tta_d4_writes_the_library_bytes(setup):
    from robosat_amd.datasets import BufferedSlippyMapDirectory
    from robosat_amd.transforms import Compose, ConvertImageMode, ImageToUint8

    s = setup
    got = _predict_in_process(s, os.path.join(s["tmp"], "probs_d4"), "d4")
    assert len(got) == 3
    directory = BufferedSlippyMapDirectory(s["tiles"], transform=Compose([ConvertImageMode(mode="RGB"), ImageToUint8()]), size=TILE,
                                           overlap=OVERLAP, mode="RGB")
    plain = _predict_in_process(s, os.path.join(s["tmp"], "probs_plain"))
    differs = 0
    for i in range(len(directory)):
        image, tile = directory[i]
        x, y, z = list(map(int, tile))
        key = os.path.join(str(z), str(x), str(y) + ".png")
        want = s["net"].predict_quantized(torch.as_tensor(np.asarray(image)).unsqueeze(0).to(DEV), overlap=OVERLAP, tta="d4")[0]
        assert np.array_equal(got[key], want.cpu().numpy()), key
        differs += int(not np.array_equal(got[key], plain[key]))
    assert differs > 0  # (TTA changed the output)


def test_predict_tta_none_writes_the_plain_files(setup):
    s = setup
    plain = _predict_in_process(s, os.path.join(s["tmp"], "probs_plain2"))
    none = _predict_in_process(s, os.path.join(s["tmp"], "probs_none"), "none")
    assert plain.keys() == none.keys() and len(plain) == 3
    for f in plain:
        assert np.array_equal(plain[f], none[f]), f


def test_predict_tta_refused_on_the_host_pipeline(setup, monkeypatch):
    s = setup
    monkeypatch.setenv("ROBOSAT_PREDICT_HOST_PIPELINE", "1")
    with pytest.raises(SystemExit, match="--tta d4"):
        _predict_in_process(s, os.path.join(s["tmp"], "probs_host"), "d4")


def test_two_rank_predict_forwards_tta(setup):
    s = setup
    outs = {}
    for name, env in (("two", {"ROBOSAT_GPUS": "2", "ROBOSAT_DIST_BACKEND": "gloo"}), ("one", {"ROBOSAT_GPUS": "1"})):
        probs = os.path.join(s["tmp"], "probs_rank_" + name)
        r = _rs(["predict", "--batch_size", "1", "--checkpoint", s["ck"], "--overlap", str(OVERLAP), "--tile_size", str(TILE), "--model",
                 s["model"], "--dataset", s["dataset"], "--tta", "d4", s["tiles"], probs], env, s["tmp"])
        assert r.returncode == 0, r.stdout + r.stderr
        outs[name] = _files(probs)
    d4 = _predict_in_process(s, os.path.join(s["tmp"], "probs_d4_again"), "d4")
    assert outs["one"].keys() == outs["two"].keys() == d4.keys() and len(d4) == 3
    for f in d4:
        assert np.array_equal(outs["two"][f], outs["one"][f]), f
        assert np.array_equal(outs["two"][f], d4[f]), f  # (a relaunch that dropped the flag would write the plain files)


def test_predictor_segment_with_tta(setup):
    from robosat_amd.tools.serve import Predictor

    s = setup
    model = {"common": {"cuda": True}}
    dataset = {"common": {"classes": ["background", "parking"], "colors": ["denim", "orange"]}}
    rng = np.random.default_rng(2)
    pixels = rng.integers(0, 256, size=(256, 256, 3), dtype=np.uint8)
    image = Image.fromarray(pixels, mode="RGB")
    mask = Predictor(s["ck"], model, dataset, tta="d4").segment(image)
    want = s["net"].predict_classes(torch.from_numpy(pixels).unsqueeze(0).to(DEV), tta="d4")[0].cpu().numpy()
    assert mask.mode == "P" and np.array_equal(np.array(mask), want)
    plain = Predictor(s["ck"], model, dataset).segment(image)  # (the three-argument form keeps working)
    assert np.array_equal(np.array(plain), s["net"].predict_classes(torch.from_numpy(pixels).unsqueeze(0).to(DEV))[0].cpu().numpy())
