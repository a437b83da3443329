"""GPU: the batched augmentation (falnet_augment_batch behind data_transforms.BatchAugment) and the HBM-resident training set
(datasets.ResidentStereoPairs) -- against the reference-made goldens, against the per-sample path (StereoAugment), against Pillow
itself, and through the training script."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import data_transforms as DT  # noqa: E402
from fal_net_amd import datasets as DS  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEV = "cuda:0"
MEAN = torch.tensor(DT.MEAN).view(3, 1, 1)
CB = [[0.8, 1.0, 1.2], [1.19, 0.81, 1.1]]
_FRAMES = {}


def frame_pair(h, w):
    """A seeded uint8 pair of one size, made once and shared (host arrays; never written)."""
    if (h, w) not in _FRAMES:
        rng = np.random.default_rng(1000 * h + w)
        _FRAMES[(h, w)] = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    return _FRAMES[(h, w)]


def to_dev(pair):
    return [torch.from_numpy(a).to(DEV) for a in pair]


def prm(h, w, th, tw, factor=None, rw=None, rh=None, x1=0, y1=0, flip=False, gamma=None, bright=None, cbright=None):
    rw = int(w * factor) if rw is None else rw
    rh = int(h * factor) if rh is None else rh
    assert rw >= tw and rh >= th, (h, w, th, tw, rw, rh)
    return dict(factor=factor, rw=rw, rh=rh, x1=rw - tw if x1 == "max" else x1, y1=rh - th if y1 == "max" else y1, flip=flip,
                gamma=gamma, bright=bright, cbright=cbright)


def small_cases(th, tw):
    """(h, w, params) over the three small frames: factor 0.75 (7 taps) and 1.5 (5 taps), an axis with rw == W, both axes unchanged, the crop
    at the origin and at the far corner (where xmin / xmax clamp at the image border), flip on and off, every colour branch."""
    return [
        (50, 171, prm(50, 171, th, tw, 0.75)),                                                      # origin, no colour transform
        (50, 171, prm(50, 171, th, tw, 0.75, x1="max", y1="max", flip=True, gamma=1.17)),            # far corner, gamma only
        (45, 150, prm(45, 150, th, tw, 1.5, x1="max", y1="max", flip=True, bright=1.9)),             # brightness that saturates
        (45, 150, prm(45, 150, th, tw, 1.5, cbright=CB)),                                           # truncating per-channel on a still-uint8 array
        (48, 160, prm(48, 160, th, tw, rw=160, rh=62, x1=5, y1="max", bright=0.7, cbright=CB)),     # rw == W; per-channel on a float array
        (48, 160, prm(48, 160, th, tw, 1.0, x1=3, y1=2, flip=True, cbright=CB)),                     # neither axis resampled
        (48, 160, prm(48, 160, th, tw, 1.23, x1=7, y1=1, gamma=0.85, bright=1.4, cbright=CB)),       # everything at once
    ]


BIG = (375, 1242)
BIG_CASES = [
    (*BIG, prm(*BIG, 192, 640, 0.75, x1="max", y1="max", flip=True, gamma=0.9)),
    (*BIG, prm(*BIG, 192, 640, 1.5, cbright=CB)),
    (*BIG, prm(*BIG, 192, 640, 1.0, x1=301, y1=90, bright=1.6, cbright=CB)),
]


def per_sample(th, tw, cases):
    aug = DT.StereoAugment(th, tw)
    outs = [aug(to_dev(frame_pair(h, w)), params=p) for h, w, p in cases]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def assert_same(got, ref, params):
    """Where gamma does not fire every operation is exact: torch.equal.  Where it fires: 2e-6.  Returns the largest difference seen."""
    worst = 0.0
    for j in range(2):
        for i, p in enumerate(params):
            d = float((got[j][i] - ref[j][i]).abs().max())
            worst = max(worst, d)
            if p["gamma"]:
                assert d <= 2e-6, (i, j, d)
            else:
                assert torch.equal(got[j][i], ref[j][i]), (i, j, d)
    return worst


def test_golden_g8_as_one_batch(golden_dir):
    """Every aug* case of g8_data_aug.npz (48 x 160 -> 32 x 96, recorded from the reference's data_transforms + Pillow) in ONE call, the
    params rebuilt by re-seeding per case: within 2e-6 of the reference's outputs, the gate of test_data_augmentation_vs_reference_goldens
    (device pow against libm in RandomGamma is the only source of a difference)."""
    g = np.load(os.path.join(golden_dir, "g8_data_aug.npz"))
    H, W, TH, TW = (int(v) for v in g["aug_shape"])
    aug = DT.BatchAugment(TH, TW)
    pairs, params = [], []
    for k, seed in enumerate(g["aug_seeds"]):
        random.seed(int(seed))
        np.random.seed(int(seed))
        params.append(aug.draw(H, W))
        pairs.append([torch.from_numpy(g[f"aug{k}_left"]).to(DEV), torch.from_numpy(g[f"aug{k}_right"]).to(DEV)])
    assert len(pairs) == len(g["aug_seeds"]) >= 8
    outs = aug(pairs, params=params)
    assert outs[0].shape == outs[1].shape == (len(pairs), 3, TH, TW)
    for k in range(len(pairs)):
        for j in range(2):
            d = float((outs[j][k].cpu() - torch.from_numpy(g[f"aug{k}_out{j}"])).abs().max())
            print(f"G8 case {k} view {j}: max |diff| {d:.3g}")
            assert d <= 2e-6, (k, j, d)


@pytest.mark.parametrize("th,tw,which", [(32, 96, "small"), (37, 101, "small"), (192, 640, "big")])
def test_batch_equals_per_sample_path(th, tw, which):
    """One batch of pairs of different sizes with explicit params through both paths: bit for bit where gamma does not fire, within 2e-6
    where it does.  37 x 101 is no multiple of the 16 x 64 tile; 192 x 640 is many tiles of a full-size frame.
    Measured maximum difference on the gamma cases (MI355X): 0 (the two kernels run the same pow on the same bytes)."""
    cases = small_cases(th, tw) if which == "small" else BIG_CASES
    params = [p for _, _, p in cases]
    ref = per_sample(th, tw, cases)
    got = DT.BatchAugment(th, tw)([to_dev(frame_pair(h, w)) for h, w, _ in cases], params=params)
    worst = assert_same(got, ref, params)
    print(f"{th} x {tw}: largest difference to the per-sample path {worst:.3g}")
    # into caller-owned tensors: the same values, and the returned tensors are the caller's
    out = (torch.full_like(ref[0], 7.0), torch.full_like(ref[1], 7.0))
    back = DT.BatchAugment(th, tw)([to_dev(frame_pair(h, w)) for h, w, _ in cases], params=params, out=out)
    assert back[0] is out[0] and back[1] is out[1] and torch.equal(out[0], got[0]) and torch.equal(out[1], got[1])


def test_integer_stage_equals_pillow():
    """No flip, no colour transform: u = rint((out + mean) * 255) recovers the resampled bytes; as integers they equal
    Image.resize((rw, rh), BICUBIC) cropped on the host -- for the small frames and for a 375 x 1242 frame at factors 0.75, 1.0, 1.5.
    Pins the device-computed coefficients and the crop-window two-pass to Pillow itself."""
    from PIL import Image
    for th, tw, cases in ((32, 96, [(50, 171, 0.75, 0, 0), (50, 171, 0.75, "max", "max"), (45, 150, 1.5, "max", "max"), (45, 150, 1.5, 0, 0),
                                    (48, 160, 1.0, 9, 4), (48, 160, 1.23, "max", 0), (48, 160, 0.9, 0, "max")]),
                          (37, 101, [(50, 171, 0.75, 0, 0), (45, 150, 1.5, "max", "max"), (48, 160, 1.37, 13, 11)]),
                          (192, 640, [(*BIG, 0.75, "max", "max"), (*BIG, 0.75, 0, 0), (*BIG, 1.0, 211, 77), (*BIG, 1.5, 0, 0), (*BIG, 1.5, "max", "max")])):
        params = [prm(h, w, th, tw, f, x1=x1, y1=y1) for h, w, f, x1, y1 in cases]
        outs = DT.BatchAugment(th, tw)([to_dev(frame_pair(h, w)) for h, w, *_ in cases], params=params)
        for i, ((h, w, *_), p) in enumerate(zip(cases, params)):
            for j in range(2):
                u = torch.round((outs[j][i].cpu().double() + MEAN.double()) * 255.0).to(torch.int64).permute(1, 2, 0).numpy()
                ref = np.array(Image.fromarray(frame_pair(h, w)[j]).resize((p["rw"], p["rh"]), Image.BICUBIC))[p["y1"]:p["y1"] + th, p["x1"]:p["x1"] + tw]
                assert np.array_equal(u, ref.astype(np.int64)), (th, tw, i, j, int(np.abs(u - ref).max()))


def test_draw_order_equals_a_loop_of_stereo_augment():
    """Seeded, B = 3, no params given: BatchAugment draws once per sample in sample order, exactly what a loop of StereoAugment draws."""
    th, tw = 32, 96
    sizes = [(48, 160), (50, 171), (45, 150)]
    for seed in (0, 5):
        random.seed(seed)
        np.random.seed(seed)
        loop = DT.StereoAugment(th, tw)
        outs = [loop(to_dev(frame_pair(h, w))) for h, w in sizes]
        ref = (torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs]))
        after = (random.random(), np.random.uniform())
        random.seed(seed)
        np.random.seed(seed)
        params = [DT.draw_params(h, w, th, tw) for h, w in sizes]
        random.seed(seed)
        np.random.seed(seed)
        got = DT.BatchAugment(th, tw)([to_dev(frame_pair(h, w)) for h, w in sizes])
        assert (random.random(), np.random.uniform()) == after  # both generators end where the loop left them
        assert_same(got, ref, params)


def test_refusals():
    """A crop outside the resized image, a factor outside the stated range [0.5, 2.0] and a CPU tensor are refused by the library
    (falnet_last_error), before any launch."""
    th, tw = 32, 96
    aug = DT.BatchAugment(th, tw)
    pair = to_dev(frame_pair(48, 160))
    good = prm(48, 160, th, tw, 1.0)
    with pytest.raises(RuntimeError, match="augment_batch.*outside the resized image"):
        aug([pair, pair], params=[good, dict(good, x1=160 - tw + 1)])
    with pytest.raises(RuntimeError, match="augment_batch.*outside the resized image"):
        aug([pair], params=[dict(good, y1=-1)])
    with pytest.raises(RuntimeError, match="augment_batch.*outside the supported scale factors"):
        aug([pair], params=[prm(48, 160, th, tw, 2.5)])
    with pytest.raises(RuntimeError, match="augment_batch.*outside the supported scale factors"):
        DT.BatchAugment(8, 8)([pair], params=[prm(48, 160, 8, 8, 0.4)])
    with pytest.raises(RuntimeError, match="augment_batch.*not device memory"):
        aug([pair, [pair[0], torch.from_numpy(frame_pair(48, 160)[1])]], params=[good, good])
    outs = aug([pair], params=[good])  # and the object still works after a refusal
    assert torch.equal(outs[0][0], DT.StereoAugment(th, tw)(pair, params=good)[0])


def _write_tree(tmp_path, sizes=((70, 200), (72, 214), (75, 190)), per_size=2):
    """<root>/Kitti/<drive>/image_0{2,3}/data/*.png of generated frames (per_size pairs of each size) + a pair list."""
    from PIL import Image
    rng = np.random.default_rng(11)
    root = tmp_path / "data"
    lines, arrays = [], []
    for i in range(len(sizes) * per_size):
        h, w = sizes[i % len(sizes)]
        pair = []
        for cam in ("image_02", "image_03"):
            d = root / "Kitti" / "2011_09_26" / "drive_0001_sync" / cam / "data"
            d.mkdir(parents=True, exist_ok=True)
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            Image.fromarray(a).save(d / f"{i:010d}.png")
            pair.append(a)
        arrays.append(pair)
        lines.append(f"2011_09_26/drive_0001_sync/image_02/data/{i:010d}.png 2011_09_26/drive_0001_sync/image_03/data/{i:010d}.png")
    lst = tmp_path / "train_pairs.txt"
    lst.write_text("\n".join(lines) + "\n")
    return root, lst, arrays


def test_resident_set(tmp_path):
    """6 pairs of three sizes decoded once into the arena: every frame reads back equal to its decoded array, a batch drawn from the
    arena equals BatchAugment on separately uploaded frames bit for bit, and an arena above the room check is refused by name and number."""
    root, lst, arrays = _write_tree(tmp_path)
    kroot = str(root / "Kitti")
    pairs = DS.read_pair_list(str(lst), kroot)
    assert len(pairs) == 6
    res = DS.ResidentStereoPairs(kroot, pairs, DEV, max_pix=300, workers=2)
    assert len(res) == 6 and res.frames.shape == (12, 3) and res.arena.dtype == torch.uint8 and res.arena.is_cuda
    for i, pair in enumerate(arrays):
        for v in range(2):
            assert tuple(res.frames[2 * i + v][1:].tolist()) == pair[v].shape[:2]
            assert np.array_equal(res.frame(i, v).cpu().numpy(), pair[v]), (i, v)
    th, tw = 64, 128
    aug = DT.BatchAugment(th, tw)
    indices = [4, 1, 5, 0]
    random.seed(3)
    np.random.seed(3)
    params = [aug.draw(*arrays[i][0].shape[:2]) for i in indices]
    params[1] = dict(params[1], flip=True, gamma=None)
    params[2] = dict(params[2], flip=False, gamma=None, bright=None, cbright=CB)
    left, right, mx = res.batch(indices, aug, params=params)
    ref = aug([to_dev(arrays[i]) for i in indices], params=params)
    assert torch.equal(left, ref[0]) and torch.equal(right, ref[1])
    assert mx.shape == (4, 1, 1) and float(mx.min()) == float(mx.max()) == 300.0
    for b in res.epoch_batches(0, 2):
        l2, r2, _ = res.batch(b, aug)  # own draws
        assert l2.shape == (2, 3, th, tw) and bool(torch.isfinite(l2).all()) and bool(torch.isfinite(r2).all())
    need = sum(-(-a.size // DS.ResidentStereoPairs.ALIGN) * DS.ResidentStereoPairs.ALIGN for p in arrays for a in p)
    with pytest.raises(MemoryError, match=rf"needs {need} bytes, more than \S+ of the \d+ bytes free"):
        DS.ResidentStereoPairs(kroot, pairs, DEV, workers=0, max_fraction=1e-9)


@pytest.mark.parametrize("mode", ["resident", "synthetic"])
def test_training_script_switches(mode, tmp_path):
    """Train_Stage1_K.py --resident-data on a generated tree, and --synthetic --gpu-augment --batch-augment: a child process under its own
    time limit, two steps at 64 x 128 with batch 2, finite-loss JSON lines, exit status 0."""
    common = ["--epochs", "1", "--epoch_size", "2", "-b", "2", "-ch", "64", "-cw", "128", "-p", "1", "--save-path", str(tmp_path / "run")]
    if mode == "resident":
        root, lst, _ = _write_tree(tmp_path)
        argv = ["-d", str(root), "--train_list", str(lst), "--resident-data", "-w", "2"]
    else:
        argv = ["--synthetic", "--gpu-augment", "--batch-augment"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "Train_Stage1_K.py")] + argv + common, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    losses = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{") and '"loss"' in line]
    assert len(losses) == 2
    for rec in losses:
        assert rec["loss"] == rec["loss"] and abs(rec["loss"]) != float("inf")
