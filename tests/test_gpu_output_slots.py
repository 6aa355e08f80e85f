"""Every output a caller can bind or read back (gbuffer x 4, ray outputs x 5, visibility x 2, denoised, motion,
upsampled, subsamples, antialiased, variance, and the half buffer), driven through the same sequence on the MI355X: read before
any write, write into the handle's own buffer, bind a tensor and read without writing, write into the tensor, un-bind, write
again.  What a read does at each step is that output's rule as the table in DESIGN.md states it; the rules differ, and
the differences are kept (the table lists them as "differs, not known to be intended").

The frame is 24 x 16 — six 8 x 8 tiles, one full workgroup of four waves and one partial — and the ray batch has 33 rays, one
partial wave.  Every comparison is bit for bit: each write of a row computes the same values, so the tensor a write went
into must equal both what the read returns and what the own buffer got from the same call earlier."""
import ctypes as C

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

W, H, RAYS = 24, 16, 33
SENTINEL = -7


def _rays():
    o = np.zeros((RAYS, 4), dtype=np.float32)
    d = np.zeros((RAYS, 4), dtype=np.float32)
    d[:, 0] = np.linspace(-0.5, 0.5, RAYS)
    d[:, 1] = np.linspace(-0.2, 0.1, RAYS)
    d[:, 2] = 1.0
    d[:, 3] = 100.0
    return o, d


def _tracer(srt, oracle):
    """Scene1 through the default camera, two samples in the accumulator and 33 rays written."""
    oarr, n = oracle.make_objects(oracle.load_scene_json_py(scene_path("Scene1")))
    pt = srt.PathTracer(W, H)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(srt.default_camera())
    pt.render(spp=2, bounces=2, seed=0)
    pt.write_rays(*_rays())
    return pt


def _vis_write(name):
    def write(pt):
        pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
        pt.render_visibility(ao_samples=4, ao=name == "ao", sun=name == "sun")
    return write


def _variance_write(pt):
    pt.half_ptr()
    pt.variance(merge=False)


def _motion_write(pt):
    pt.motion_output(True)
    pt.temporal(reset=True)


# name -> (shape, dtype, write, read, bind, what a read gives after a bind without a write, ... after the un-bind)
#   "bound": the tensor's contents     "own": the own buffer's contents     "last": the buffer the last write went to
#   "state": SRT_ERR_STATE
def _rows():
    rows = {}
    for name, ch, dt in (("object", 1, np.int32), ("normal_depth", 4, np.float32), ("position", 4, np.float32), ("albedo", 4, np.float32)):
        px = (H, W) if ch == 1 else (H, W, ch)
        rows["gbuffer:" + name] = (px, dt, lambda pt, n=name: pt.render_gbuffer(outputs=[n]), lambda pt, n=name: pt.gbuffer(n),
                                   lambda pt, t, n=name: pt.bind_gbuffer(n, t), "bound", "own")
    for name, ch, dt in (("object", 1, np.int32), ("normal_depth", 4, np.float32), ("position", 4, np.float32), ("albedo", 4, np.float32),
                         ("occluded", 1, np.int32)):
        rows["rays:" + name] = ((RAYS,) if ch == 1 else (RAYS, ch), dt, lambda pt, n=name: pt.trace_rays(outputs=[n]),
                                lambda pt, n=name: pt.ray_output(n, count=RAYS), lambda pt, t, n=name: pt.bind_ray_output(n, t), "last", "last")
    for name in ("ao", "sun"):
        rows["visibility:" + name] = ((H, W), np.float32, _vis_write(name), lambda pt, n=name: pt.visibility(n),
                                      lambda pt, t, n=name: pt.bind_visibility(n, t), "last", "last")
    f4 = (H, W, 4)
    rows["denoised"] = (f4, np.float32, lambda pt: pt.denoise(iterations=2), lambda pt: pt.denoised(), lambda pt, t: pt.bind_denoised(t), "bound", "own")
    rows["motion"] = (f4, np.float32, _motion_write, lambda pt: pt.motion(), lambda pt, t: pt.bind_motion(t), "state", "state")
    rows["upsampled"] = (f4, np.float32, lambda pt: pt.upsample(), lambda pt: pt.upsampled(), lambda pt, t: pt.bind_upsampled(t), "bound", "own")
    rows["subsamples"] = ((4, H, W), np.int32, lambda pt: pt.render_subsamples(k=2), lambda pt: pt.subsamples(k=2),
                          lambda pt, t: pt.bind_subsamples(t), "bound", "own")
    rows["antialiased"] = (f4, np.float32, lambda pt: pt.antialias(k=2), lambda pt: pt.antialiased(), lambda pt, t: pt.bind_antialiased(t), "bound", "own")
    rows["variance"] = ((H, W), np.float32, _variance_write, lambda pt: pt.variance_map(), lambda pt, t: pt.bind_variance(t), "bound", "own")
    return rows


ROWS = _rows()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _expect(srt, pt, read, rule, tensor_now, own, what):
    if rule == "state":
        with pytest.raises(srt.SrtError) as e:
            read(pt)
        assert e.value.code == srt.capi.ERR_STATE, what
        return
    want = tensor_now if rule == "bound" or (rule == "last" and tensor_now is not None) else own
    got = read(pt)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), what


@pytest.mark.parametrize("name", list(ROWS))
def test_output_slot(srt, oracle, name):
    import torch

    shape, dtype, write, read, bind, after_bind, after_unbind = ROWS[name]
    sentinel = np.full(shape, SENTINEL, dtype=dtype)
    with _tracer(srt, oracle) as pt:
        # nothing written, nothing bound
        with pytest.raises(srt.SrtError) as e:
            read(pt)
        assert e.value.code == srt.capi.ERR_STATE, name
        # a write into the own buffer
        write(pt)
        own = read(pt)
        assert own.shape == shape and own.dtype == dtype and not np.array_equal(_bits(own), _bits(sentinel)), name
        # a tensor bound, not yet written ("last": the last write went to the own buffer)
        t = torch.full(shape, SENTINEL, dtype=torch.int32 if dtype == np.int32 else torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        bind(pt, t)
        _expect(srt, pt, read, after_bind, sentinel if after_bind == "bound" else None, own, name + ": bound, not written")
        # a write into the tensor: the tensor, the read and the own buffer's earlier copy agree bit for bit
        write(pt)
        pt.wait()
        got = t.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(own)), name + ": the tensor does not hold what the own buffer got"
        assert np.array_equal(_bits(read(pt)), _bits(got)), name + ": the read differs from the bound tensor"
        # un-bound: the tensor is overwritten first, so a read that still goes to it shows
        t.fill_(SENTINEL)
        torch.cuda.synchronize()
        bind(pt, None)
        _expect(srt, pt, read, after_unbind, sentinel if after_unbind == "last" else None, own, name + ": un-bound")
        # ... and the next write goes to the own buffer again, whatever the rule
        write(pt)
        assert np.array_equal(_bits(read(pt)), _bits(own)), name + ": written again"
        torch.cuda.synchronize()
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(sentinel)), name + ": the un-bound tensor was written"


def test_half_buffer(srt, oracle):
    """srt_device_half / srt_bind_half have no read: srt_variance shows which buffer is half B.  The own one starts as zeros, so
    the variance against it is not zero; a bound copy of the accumulator gives exactly zero everywhere."""
    import torch

    with _tracer(srt, oracle) as pt:
        with pytest.raises(srt.SrtError) as e:  # neither bound nor fetched
            pt.variance(merge=False)
        assert e.value.code == srt.capi.ERR_STATE
        p = pt.half_ptr()
        assert p and pt.half_ptr() == p
        pt.variance(merge=False)
        own = pt.variance_map()
        assert own.any()
        t = torch.from_numpy(pt.accumulator()).to("cuda:0")
        torch.cuda.synchronize()
        pt.bind_half(t)
        pt.variance(merge=False)
        assert not pt.variance_map().any()
        assert pt.half_ptr() == p  # (the own buffer stays where it is while another is bound)
        pt.bind_half(None)
        pt.variance(merge=False)
        assert np.array_equal(_bits(pt.variance_map()), _bits(own))
