"""CPU: what views.sweep, freeview.warp and confidence.stats share (fal_net_amd/med_logits.py) -- every shared refusal raises the exception
type and the full message recorded from the wrappers before the checks were written once, before the library is reached; and the
split-into-launches loop on its own, with a fake launch and host tensors.  No GPU."""
import pytest
import torch

from fal_net_amd import _lib as L
from fal_net_amd import confidence, freeview, med_logits, views

POSE = freeview.pose(freeview.camera(4, 8))


def _call(who, dl, left, mn, mx):
    if who == "views.sweep":
        return views.sweep(dl, left, mn, mx, (0.5,))
    if who == "freeview.warp":
        return freeview.warp(dl, left, mn, mx, [POSE])
    return confidence.stats(dl, mn, mx)


def z(*shape):
    return torch.zeros(*shape)


# (dlog0, left, min_disp, max_disp) shapes; every tensor lives on the host, which is what the last check refuses
GOOD = ((1, 5, 4, 8), (1, 3, 4, 8), (1,), (1,))
RANK = ((5, 4, 8), (1, 3, 4, 8), (1,), (1,))
N1 = ((1, 1, 4, 8), (1, 3, 4, 8), (1,), (1,))
N129 = ((1, 129, 4, 8), (1, 3, 4, 8), (1,), (1,))
LEFT = ((1, 5, 4, 8), (1, 2, 4, 8), (1,), (1,))
EMPTY = ((1, 5, 0, 8), (1, 3, 0, 8), (1,), (1,))
MIN_DISP = ((1, 5, 4, 8), (1, 3, 4, 8), (2,), (1,))
WITH_LEFT = "{}: expected dlog0 (B, N, H, W) and left (B, 3, H, W), got (5, 4, 8) and (1, 3, 4, 8)"
REFUSALS = [
    (RANK, "views.sweep", ValueError, WITH_LEFT.format("views.sweep")),
    (RANK, "freeview.warp", ValueError, WITH_LEFT.format("freeview.warp")),
    (RANK, "confidence.stats", ValueError, "confidence.stats: expected dlog0 (B, N, H, W), got (5, 4, 8)"),
    (LEFT, "views.sweep", ValueError, "views.sweep: left (1, 2, 4, 8) does not match the logits (1, 5, 4, 8)"),
    (LEFT, "freeview.warp", ValueError, "freeview.warp: left (1, 2, 4, 8) does not match the logits (1, 5, 4, 8)"),
    (EMPTY, "views.sweep", ValueError, "views.sweep: left (1, 3, 0, 8) does not match the logits (1, 5, 0, 8)"),
    (EMPTY, "freeview.warp", ValueError, "freeview.warp: left (1, 3, 0, 8) does not match the logits (1, 5, 0, 8)"),
    (EMPTY, "confidence.stats", ValueError, "confidence.stats: empty logits (1, 5, 0, 8)"),
]
for _who in ("views.sweep", "freeview.warp", "confidence.stats"):
    REFUSALS += [
        (N1, _who, ValueError, _who + ": N=1 outside [2, 128]"),
        (N129, _who, ValueError, _who + ": N=129 outside [2, 128]"),
        (MIN_DISP, _who, ValueError, _who + ": min_disp / max_disp must hold one value per sample (B=1)"),
        (GOOD, _who, RuntimeError, "fal_net_amd.{} runs on an MI355X only (no CPU fallback); dlog0 is on cpu".format(_who.split(".")[0])),
    ]


@pytest.mark.parametrize("shapes,who,exc,msg", REFUSALS, ids=[m for _, _, _, m in REFUSALS])
def test_shared_refusals_keep_type_and_text_and_launch_nothing(monkeypatch, shapes, who, exc, msg):
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("the library was reached"))
    monkeypatch.setattr(L, "stream_ptr", lambda: pytest.fail("the stream was asked for"))
    with pytest.raises(exc) as e:
        _call(who, *(z(*s) for s in shapes))
    assert str(e.value) == msg


def test_plane_limit_is_one_object():
    assert views.MAX_PLANES == freeview.MAX_PLANES == confidence.MAX_PLANES == med_logits.MAX_PLANES == 128


def _fake_launch(log):
    def launch(part, bufs):
        log.append((list(part), bufs))
        for t in (bufs.values() if isinstance(bufs, dict) else bufs):
            if t is not None:
                assert t.shape[1] == len(part)
                for i, item in enumerate(part):
                    t[:, i] = float(item)
    return launch


@pytest.mark.parametrize("V", (1, 8, 11))
@pytest.mark.parametrize("form", ("tuple", "dict"))
def test_split_loop(V, form):
    """Limit 8.  V <= 8: one launch straight into the result tensors.  V = 11: launches of 8 and 3 items in order, into parts that are not
    the results, copied to the disjoint slices [0, 8) and [8, 11).  A None entry of a tuple stays None in every launch."""
    items = [float(10 + i) for i in range(V)]
    a, b = torch.full((2, V, 3, 2, 2), -1.0), torch.full((2, V, 1, 2, 2), -1.0)
    outs = (a, None, b) if form == "tuple" else {"view": a, "cover": b}
    log = []
    med_logits.launch_in_parts(items, 8, outs, _fake_launch(log))
    assert [p for p, _ in log] == ([items] if V <= 8 else [items[:8], items[8:]])
    for part, bufs in log:
        got = bufs if form == "tuple" else (bufs["view"], None, bufs["cover"])
        assert type(bufs) is type(outs) and got[1] is None
        if V <= 8:
            assert got[0] is a and got[2] is b
        else:
            assert got[0] is not a and got[2] is not b
            assert got[0].shape == (2, len(part), 3, 2, 2) and got[2].shape == (2, len(part), 1, 2, 2)
            assert got[0].dtype == a.dtype and got[0].device == a.device
    want = torch.tensor(items)
    assert torch.equal(a, want.view(1, V, 1, 1, 1).expand_as(a)) and torch.equal(b, want.view(1, V, 1, 1, 1).expand_as(b))
