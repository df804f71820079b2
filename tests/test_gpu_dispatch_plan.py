"""The library dispatches frames as csrc/dispatch_plan.h plans them.

tests/golden/launch_matrix.json holds RT_DEBUG_LAST_LAUNCH (up to " lpt:") of
C2 frames at 4 spp, depth 8, whose tile counts sit on or straddle the plan's
thresholds (24,000 / 40,000 / 70,000 tiles), recorded on an MI355X from the
commit before the plan existed (run_case below, three times).  Every frame
here must launch the same instance with the same split shape.  A `sky=*` in
the table marks a count that differed between two recordings: it depends on
whether the last sort's sky count had reached the host when the frame was
enqueued.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_matrix.json")
RES = [(96, 54), (640, 600), (640, 604), (800, 800), (800, 804), (1120, 1000), (1120, 1004)]
# 96x54 only: (name, frame changes, params)
EXTRA = [("band0of2", {}, dict(band_index=0, band_count=2, band_rows=8)), ("batch2", {}, {}),
         ("spp16", dict(spp=16), {}), ("depth40", dict(max_bounces=40), {}), ("count", {}, dict(flags=1))]
CASES = [f"{w}x{h}/{how}" for w, h in RES for how in ("sync", "async")] + [f"96x54/{e[0]}" for e in EXTRA]


def head(launch):
    return launch.split(" lpt:")[0]


def run_case(rt, case):
    """The case's three launches (head of last_launch each) and, for
    synchronous frames, the first and third frame's pixels."""
    import torch
    res, how = case.split("/")
    w, h = map(int, res.split("x"))
    extra = {e[0]: e for e in EXTRA}.get(how, (how, {}, {}))
    fr = rt.make("C2").with_resolution(w, h).with_(**dict(dict(spp=4, max_bounces=8), **extra[1]))
    ctx = rt.Context()  # its own longest-first slots: a case starts from no order
    launches, imgs = [], []
    try:
        ctx.set_scene(fr.scene)
        nbuf = 2 if how in ("async", "batch2") else 1
        outs = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(nbuf)]
        nbytes = outs[0].numel() * 4
        if how == "async":
            streams = [torch.cuda.Stream() for _ in range(2)]
            pa = rt.frame_params(fr, flags=rt.abi.RT_FLAG_ASYNC)
            for k in range(3):
                ctx.set_stream(streams[k % 2].cuda_stream)
                ctx.render_device(fr.camera, fr.plane, pa, outs[k % 2].data_ptr(), nbytes)
                launches.append(head(ctx.last_launch()))
            ctx.finish()
            ctx.set_stream(None)
        else:
            p = rt.frame_params(fr, **extra[2])
            for k in range(3):
                if how == "batch2":
                    buf = torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda")
                    ctx.render_device_batch([fr.camera] * 2, fr.plane, p, buf.data_ptr(), nbytes)
                    outs[0] = buf
                else:
                    ctx.render_device(fr.camera, fr.plane, p, outs[0].data_ptr(), nbytes)
                launches.append(head(ctx.last_launch()))
                imgs.append(outs[0].cpu().numpy())
        torch.cuda.synchronize()
    finally:
        ctx.close()
    return launches, imgs


def masked(got, want):
    """got with its sky count starred where the table's is."""
    return got.split(" sky=")[0] + " sky=*" if want.endswith(" sky=*") else got


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("case", CASES)
def test_launches_equal_the_recorded_matrix(gpu_ctx, rt, golden, case):
    launches, imgs = run_case(rt, case)
    want = golden[case]
    assert len(want) == 3
    assert [masked(g, w) for g, w in zip(launches, want)] == want
    if imgs:  # frame 0 measures in row order; frame 2 runs by the plan's order and splits
        assert np.array_equal(imgs[0].view(np.uint32), imgs[2].view(np.uint32)), case


def test_matrix_names_every_case(golden):
    assert sorted(golden) == sorted(CASES)
