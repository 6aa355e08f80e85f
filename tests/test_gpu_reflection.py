"""The reflection guides (srt_render_reflection_gbuffer, ABI 7) on the MI355X.  Every comparison is bit for bit over every pixel,
NaN as its bits.  The pass is held against the definition restated on the CPU (tests/reflection_reference.py: the oracle's hits,
numpy binary32 for everything between them), against a chain built on the host from the library's own pieces
(srt_render_gbuffer, reflected rays in numpy binary32, srt_trace_rays), and against srt_render_gbuffer where nothing reflects;
then bands, binding, state, the work record with the bound the lane pool must keep, and the guides' way into srt_denoise."""
import ctypes as C

import numpy as np
import pytest

import reflection_reference as RR
from conftest import scene_path
from test_gpu_radiance import moved_camera

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["object", "normal_depth", "position", "albedo", "bounces"]
GUIDES = NAMES[:4]
FRAMES = [(24, 20), (21, 13)]  # 21 x 13: partial tiles on both edges, a partial workgroup
MIRROR = dict(smoothness=1.0, specular_amount=1.0)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def json_scene(name):
    return lambda oracle: (oracle.load_scene_json_py(scene_path(name)), None)


def empty_scene(oracle):
    return [], None


def memory_scene(oracle):
    """tests/test_gpu_visibility.py's: Scene1 and a sphere whose r * r lies below 2^-72, so the scene is read from memory
    (SCENE_LDS == false)."""
    objs = oracle.load_scene_json_py(scene_path("Scene1"))
    objs.append(dict(type=oracle.OBJ_SPHERE, position=(0.0, 100.0, -50.0), radius=1e-12, base=(.9, .2, .1)))
    return objs, None


def mirror_mesh_scene(oracle):
    """A mirror UV sphere (2 * 20 * 15 triangles) and a mirror ball over a diffuse floor, a diffuse ball next to them."""
    objs = [dict(type=oracle.OBJ_MESH, position=(0.0, 0.0, 5.0), mesh=0, base=(0.8, 0.3, 0.2), specular=(0.9, 0.8, 0.7), **MIRROR),
            dict(type=oracle.OBJ_BOX, position=(0.0, -1.5, 5.0), half_size=(6.0, 0.5, 6.0), base=(0.6, 0.6, 0.6)),
            dict(type=oracle.OBJ_SPHERE, position=(1.6, -0.6, 4.2), radius=0.4, base=(0.2, 0.4, 0.9), specular=(0.5, 0.6, 0.7), **MIRROR),
            dict(type=oracle.OBJ_SPHERE, position=(-1.7, -0.5, 4.4), radius=0.5, base=(0.1, 0.7, 0.2))]
    return objs, [oracle.uv_sphere(1.0, 16, 20)]


SCENES = {"Scene1_reflection": json_scene("Scene1_reflection"), "Scene3": json_scene("Scene3"), "Scene_indirect": json_scene("Scene_indirect"),
          "Scene1": json_scene("Scene1"), "empty": empty_scene, "memory": memory_scene, "mirror_mesh": mirror_mesh_scene}
CAMERAS = {"default": lambda oracle: oracle.default_camera(), "moved": moved_camera}


class Frame:
    """A tracer with a scene and a camera; the oracle's copy of both."""

    def __init__(self, srt, oracle, scene, w, h, cam=None):
        objs, meshes = scene
        self.srt, self.oracle, self.w, self.h = srt, oracle, w, h
        self.oarr, self.n = oracle.make_objects(objs)
        self.pt = srt.PathTracer(w, h)
        self.om = None
        if meshes:
            marr, mn, keep = oracle.make_meshes(meshes)
            self.pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
            self.om = (marr, mn, keep)
        self.pt.set_scene(C.cast(self.oarr, C.POINTER(srt.Object)), self.n)
        self.ocam = cam if cam is not None else oracle.default_camera()
        self.pt.set_camera(C.cast(C.pointer(self.ocam), C.POINTER(srt.Camera)).contents)

    def reference(self, **kw):
        return RR.reference(self.oracle, self.oarr, self.n, self.ocam, self.w, self.h, om=self.om, **kw)

    def render(self, **kw):
        self.pt.render_reflection_gbuffer(**kw)
        return {k: self.pt.read_reflection(k) for k in NAMES}

    def close(self):
        self.pt.close()


def assert_same(got, want, names=NAMES, what=""):
    for k in names:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        diff = a.view(np.uint32) != b.view(np.uint32)
        assert not diff.any(), "%s %s differs at %d of %d elements, first at %s" % (what, k, int(diff.sum()), diff.size, np.argwhere(diff)[0])


# ---- 1. against the CPU reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_against_the_cpu_reference(srt, oracle, scene, camera, size):
    fr = Frame(srt, oracle, SCENES[scene](oracle), *size, cam=CAMERAS[camera](oracle))
    try:
        got, want = fr.render(), fr.reference()
        on, off = RR.histogram(want)
        print(scene, camera, size, "ends on an object", on, "leaves the scene", off)
        assert_same(got, want, what="%s %s %dx%d" % ((scene, camera) + size))
        if scene == "Scene1_reflection" and camera == "default" and size == (24, 20):
            assert all(on.get(J, 0) > 0 for J in (0, 1, 2, 3, 8)) and all(off.get(J, 0) > 0 for J in range(9))
        if scene == "mirror_mesh":  # the mesh and the sphere do reflect: chains that end on an object after one and two reflections
            assert on.get(1, 0) > 0 and (camera != "default" or size != (24, 20) or on.get(2, 0) > 0)
        if scene in ("Scene1", "memory", "empty"):
            assert not got["bounces"].any()
    finally:
        fr.close()


# ---- 2. against the library's own pieces -----------------------------------------------------------------------------------------
def host_chain(fr, max_bounces, min_smoothness=1.0, min_specular=1.0):
    """The chain built on the host step by step: srt_render_gbuffer, then reflected rays in numpy binary32 (one IEEE operation per
    statement) and srt_trace_rays on exactly the continuing pixels, repeated until none continues."""
    pt, n_px = fr.pt, fr.w * fr.h
    pt.render_gbuffer()
    cur = {k: pt.gbuffer(k).reshape((n_px,) + ((4,) if k != "object" else ())).copy() for k in GUIDES}
    mats = [fr.oarr[i].material for i in range(fr.n)]
    smooth = np.array([m.smoothness for m in mats] + [np.nan], F)  # (index -1: a miss follows nothing)
    amount = np.array([m.specular_amount for m in mats] + [np.nan], F)
    base = np.array([[RR.c0(v) for v in m.base_color] for m in mats] + [[0, 0, 0]], F).reshape(-1, 3)
    spec = np.array([[RR.c0(v) for v in m.specular_color] for m in mats] + [[0, 0, 0]], F).reshape(-1, 3)
    # per pixel: the direction of the ray that made the current hit
    L = fr.oracle.lib()
    d3 = (C.c_float * 3)()
    d = np.empty((n_px, 3), F)
    for y in range(fr.h):
        for x in range(fr.w):
            L.srt_oracle_ray_direction(C.byref(fr.ocam), fr.w, fr.h, x, y, d3)
            d[x + y * fr.w] = d3[:]
    J = np.zeros(n_px, np.int32)
    D = cur["normal_depth"][:, 3].copy()
    T = np.zeros((n_px, 3), F)
    alive = np.ones(n_px, bool)  # the pixel's chain has not stopped
    while True:
        o = cur["object"]
        with np.errstate(invalid="ignore"):
            go = alive & (o != -1) & (J < max_bounces) & (smooth[o] >= F(min_smoothness)) & (amount[o] >= F(min_specular))
        alive = go
        if not go.any():
            break
        ix = np.flatnonzero(go)
        first = J[ix] == 0
        T[ix] = np.where(first[:, None], base[o[ix]], (T[ix] * spec[o[ix]]).astype(F))
        n, p, dd = cur["normal_depth"][ix, :3], cur["position"][ix, :3], d[ix]
        a = (dd[:, 0] * n[:, 0]).astype(F)
        b = (dd[:, 1] * n[:, 1]).astype(F)
        ab = (a + b).astype(F)
        c = (dd[:, 2] * n[:, 2]).astype(F)
        k = (F(2.0) * (ab + c).astype(F)).astype(F)
        r = (dd - (n * k[:, None]).astype(F)).astype(F)
        xx = (r[:, 0] * r[:, 0]).astype(F)
        yy = (r[:, 1] * r[:, 1]).astype(F)
        s = (xx + yy).astype(F)
        zz = (r[:, 2] * r[:, 2]).astype(F)
        with np.errstate(invalid="ignore", divide="ignore"):
            length = np.sqrt((s + zz).astype(F)).astype(F)
            r = (r / length[:, None]).astype(F)
        org = (p + (n * F(.00001)).astype(F)).astype(F)
        O4, D4 = np.zeros((len(ix), 4), F), np.zeros((len(ix), 4), F)
        O4[:, :3], D4[:, :3], D4[:, 3] = org, r, np.inf
        pt.write_rays(O4, D4)
        pt.trace_rays(outputs=GUIDES)
        hit = {k: pt.ray_output(k) for k in GUIDES}
        d[ix] = r
        J[ix] += 1
        for k in GUIDES:
            cur[k][ix] = hit[k]
        landed = hit["object"] != -1
        t = hit["normal_depth"][:, 3]
        D[ix] = np.where(landed, (D[ix] + t).astype(F), F(np.inf))
        cur["normal_depth"][ix, 3] = D[ix]
        later = landed & (J[ix] >= 2)
        T[ix] = np.where(later[:, None], (T[ix] * F(0.8)).astype(F), T[ix])
        alb = np.where(landed[:, None], (T[ix] * base[hit["object"]]).astype(F), F(0.0))
        cur["albedo"][ix, :3] = alb
    shape = lambda k: (fr.h, fr.w) if k in ("object", "bounces") else (fr.h, fr.w, 4)
    out = {k: cur[k].reshape(shape(k)) for k in GUIDES}
    out["bounces"] = J.reshape(fr.h, fr.w)
    return out


@pytest.fixture(scope="module")
def reflection_frame(srt, oracle):
    fr = Frame(srt, oracle, SCENES["Scene1_reflection"](oracle), 24, 20)
    yield fr
    fr.close()


@pytest.mark.parametrize("max_bounces", [0, 1, 3, 8, 64])
def test_against_a_chain_built_from_gbuffer_and_trace_rays(reflection_frame, max_bounces):
    fr = reflection_frame
    want = host_chain(fr, max_bounces)
    got = fr.render(max_bounces=max_bounces)
    print("max_bounces", max_bounces, "J histogram", np.bincount(got["bounces"].reshape(-1)).tolist())
    assert_same(got, want, what="max_bounces %d" % max_bounces)
    assert int(got["bounces"].max()) == (min(max_bounces, 8) if max_bounces < 64 else int(want["bounces"].max()))
    if max_bounces == 64:
        assert int(got["bounces"].max()) > 8  # chains the default cuts short go on


# ---- 3. identity ------------------------------------------------------------------------------------------------------------------
def test_identity_where_nothing_is_followed(srt, oracle, reflection_frame):
    inf = float("inf")
    cases = [(reflection_frame, dict(max_bounces=0)), (reflection_frame, dict(min_smoothness=inf)), (reflection_frame, dict(min_specular=inf)),
             (reflection_frame, dict(min_smoothness=inf, min_specular=inf, max_bounces=64))]
    scene1 = Frame(srt, oracle, SCENES["Scene1"](oracle), 21, 13)
    try:
        for fr, kw in cases + [(scene1, {})]:
            got = fr.render(**kw)
            fr.pt.render_gbuffer()
            assert_same(got, {k: fr.pt.gbuffer(k) for k in GUIDES}, names=GUIDES, what=str(kw))
            assert not got["bounces"].any()
    finally:
        scene1.close()


# ---- 4. thresholds ----------------------------------------------------------------------------------------------------------------
def test_thresholds_follow_glossy_materials(srt, oracle):
    objs, _ = SCENES["Scene3"](oracle)
    smooth = sorted({round(float(o.get("smoothness", 0.5)), 3) for o in objs})
    assert 0.754 in smooth and 0.385 in smooth, smooth
    fr = Frame(srt, oracle, (objs, None), 24, 20)
    try:
        kw = dict(min_smoothness=0.7, min_specular=0.0)
        got, want = fr.render(**kw), fr.reference(**kw)
        assert_same(got, want, what="min_smoothness 0.7")
        first = fr.render(max_bounces=0)["object"]
        s_of = np.array([fr.oarr[i].material.smoothness for i in range(fr.n)] + [np.nan], F)
        s_first = s_of[first]
        is754, is385 = np.abs(s_first - F(0.754)) < 1e-3, np.abs(s_first - F(0.385)) < 1e-3
        assert is754.any() and is385.any()
        assert (got["bounces"][is754] >= 1).all() and (got["bounces"][is385] == 0).all()
        assert not RR.same_bits(got["bounces"], fr.render()["bounces"])  # the defaults follow fewer
    finally:
        fr.close()


# ---- 5. bands, binding, state -----------------------------------------------------------------------------------------------------
def test_bands_binding_and_own_buffers(srt, oracle, reflection_frame):
    import torch

    fr = reflection_frame
    pt, w, h = fr.pt, fr.w, fr.h
    whole = fr.render()
    again = fr.render()
    assert_same(again, whole, what="two calls")
    # three bands whose union is the frame, into sentinel-filled bound tensors: each writes its scene rows only
    SENT_I, SENT_F = -77, -7.0
    t = {k: (torch.full((h, w), SENT_I, dtype=torch.int32, device="cuda:0") if k in ("object", "bounces")
             else torch.full((h, w, 4), SENT_F, dtype=torch.float32, device="cuda:0")) for k in NAMES}
    for k in NAMES:
        pt.bind_reflection(k, t[k])
    done = np.zeros(h, bool)
    for rb, re in ((7, 15), (0, 7), (15, 20)):
        pt.render_reflection_gbuffer(rows=(rb, re))
        pt.wait()
        done[h - re:h - rb] = True  # memory rows [rb, re) are scene rows [H - re, H - rb)
        for k in NAMES:
            a = t[k].cpu().numpy()
            assert RR.same_bits(a[done], whole[k][done]), (k, rb, re)
            assert (a[~done] == (SENT_I if k in ("object", "bounces") else SENT_F)).all(), (k, rb, re)
            assert RR.same_bits(pt.read_reflection(k), a)  # the read copies the bound buffer
    assert done.all()
    # back to the own buffers: they still hold the whole frame of the earlier calls, and a call into a bound tensor leaves them alone
    for k in NAMES:
        pt.bind_reflection(k, None)
    for k in NAMES:
        assert RR.same_bits(pt.read_reflection(k), whole[k]), k
        view = torch.full(whole[k].shape, 3, dtype=torch.int32 if k in ("object", "bounces") else torch.float32, device="cuda:0")
        pt.bind_reflection(k, view)
        pt.render_reflection_gbuffer(outputs=[k])
        pt.bind_reflection(k, None)  # (does not wait: the enqueued launch keeps the tensor it was given)
        pt.wait()
        assert RR.same_bits(view.cpu().numpy(), whole[k])
        assert RR.same_bits(pt.read_reflection(k), whole[k])
    # a subset of the outputs writes only those
    sub = Frame(srt, oracle, SCENES["Scene1_reflection"](oracle), 24, 20)
    try:
        sub.pt.render_reflection_gbuffer(outputs=["bounces"])
        assert RR.same_bits(sub.pt.read_reflection("bounces"), whole["bounces"])
        for k in GUIDES:
            with pytest.raises(srt.SrtError) as e:
                sub.pt.read_reflection(k)
            assert e.value.code == srt.capi.ERR_STATE
    finally:
        sub.close()


def test_device_reflection_is_the_buffer_the_reads_copy_from(srt, oracle, reflection_frame):
    """The address srt_device_reflection gives, bound into a G-buffer slot of the same element type, reads back what
    srt_read_reflection reads: this is use_reflection_guides()'s plumbing.  Before the first render the buffer exists and is zero."""
    fresh = Frame(srt, oracle, SCENES["Scene1_reflection"](oracle), 24, 20)
    try:
        for k in NAMES:
            ptr = fresh.pt.reflection_ptr(k)
            assert ptr and ptr == fresh.pt.reflection_ptr(k)
            assert not fresh.pt.read_reflection(k).any()
    finally:
        fresh.close()
    fr = reflection_frame
    pt = fr.pt
    whole = fr.render()
    try:
        for k in NAMES:
            slot = "object" if k == "bounces" else k
            ptr = pt.reflection_ptr(k)
            assert ptr and ptr == pt.reflection_ptr(k)
            pt._ck(pt.L.srt_bind_gbuffer(pt._h, srt.capi.GBUFFERS[slot][0], C.c_void_p(ptr)))
            assert RR.same_bits(pt.gbuffer(slot), whole[k]), k
            pt._ck(pt.L.srt_bind_gbuffer(pt._h, srt.capi.GBUFFERS[slot][0], None))
    finally:
        pt.use_reflection_guides(False)


def test_error_table(srt, oracle):
    c = srt.capi
    pt = srt.PathTracer(24, 20)
    try:
        def call(**kw):
            try:
                pt.render_reflection_gbuffer(**kw)
            except srt.SrtError as e:
                return e.code
            return c.OK

        assert call() == c.ERR_STATE  # no scene
        oarr, n = oracle.make_objects(oracle.load_scene_json_py(scene_path("Scene1")))
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        assert call() == c.ERR_STATE and "srt_set_camera" in str(pt.L.srt_last_error(pt._h))  # no camera
        assert call(outputs=0, max_bounces=65) == c.ERR_STATE  # ... before any argument
        pt.set_camera(srt.default_camera())
        nan, inf = float("nan"), float("inf")
        bad = [dict(rows=(0, 0)), dict(rows=(5, 5)), dict(rows=(6, 5)), dict(rows=(-1, 5)), dict(rows=(0, 21)), dict(outputs=0), dict(outputs=32),
               dict(outputs=63), dict(flags=2), dict(flags=0x80000000), dict(reserved=1), dict(max_bounces=-1), dict(max_bounces=65),
               dict(min_smoothness=nan), dict(min_specular=nan)]
        for kw in bad:
            assert call(**kw) == c.ERR_INVALID_ARG, kw
        # nothing was touched: no output exists yet
        for k in NAMES:
            with pytest.raises(srt.SrtError) as e:
                pt.read_reflection(k)
            assert e.value.code == c.ERR_STATE
        with pytest.raises(srt.SrtError) as e:
            pt.reflection_work()
        assert e.value.code == c.ERR_STATE
        good = [dict(max_bounces=0), dict(max_bounces=64), dict(min_smoothness=inf), dict(min_specular=-inf), dict(rows=(19, 20)), dict(outputs=16)]
        for kw in good:
            assert call(**kw) == c.OK, kw
        for fn in (pt.L.srt_bind_reflection, ):
            for out in (0, 3, 32):
                assert fn(pt._h, out, None) == c.ERR_INVALID_ARG
        buf = np.empty(24 * 20 * 4, F)
        p = C.c_void_p()
        for out in (0, 3, 32):
            assert pt.L.srt_read_reflection(pt._h, out, buf.ctypes.data_as(C.c_void_p)) == c.ERR_INVALID_ARG
            assert pt.L.srt_device_reflection(pt._h, out, C.byref(p)) == c.ERR_INVALID_ARG
        # srt_render_gbuffer keeps refusing the new bit
        with pytest.raises(srt.SrtError) as e:
            pt.render_gbuffer(outputs=16)
        assert e.value.code == c.ERR_INVALID_ARG
    finally:
        pt.close()


def test_the_pass_leaves_everything_else_alone(srt, oracle):
    fr = Frame(srt, oracle, SCENES["Scene1_reflection"](oracle), 24, 20)
    try:
        pt = fr.pt
        render = dict(spp=2, bounces=4, seed=5)
        pt.render(**render)
        pt.render_gbuffer()
        acc, fb = pt.accumulator(), pt.framebuffer()
        gb = {k: pt.gbuffer(k) for k in GUIDES}
        snap = lambda s: tuple(getattr(s, n) for n, _ in s._fields_)
        before = snap(pt.stats())
        fr.render(count_work=True)
        assert snap(pt.stats()) == before
        assert RR.same_bits(pt.accumulator(), acc) and np.array_equal(pt.framebuffer(), fb)
        assert_same({k: pt.gbuffer(k) for k in GUIDES}, gb, names=GUIDES, what="G-buffer slots")
        pt.render(**render)
        assert RR.same_bits(pt.accumulator(), acc) and np.array_equal(pt.framebuffer(), fb)
        after = snap(pt.stats())
        assert after[:2] == before[:2] and after[3:] == before[3:]  # (all but kernel_ms: the launch shape of the later render is the earlier one's)
    finally:
        fr.close()


# ---- 6. the work record -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["Scene3", "Scene1_reflection"])
def test_work_record_and_the_bound_of_the_lane_pool(srt, oracle, scene):
    w, h = 64, 48
    fr = Frame(srt, oracle, SCENES[scene](oracle), w, h)
    try:
        pt = fr.pt
        with pytest.raises(srt.SrtError) as e:
            pt.reflection_work()
        assert e.value.code == srt.capi.ERR_STATE
        for rows, max_bounces in (((0, h), 8), ((5, 30), 8), ((0, h), 2), ((0, h), 0)):
            got = fr.render(rows=rows, max_bounces=max_bounces, count_work=True)
            work = pt.reflection_work()
            band = slice(h - rows[1], h - rows[0])
            n_rows = rows[1] - rows[0]
            tiles = ((w + 7) // 8) * ((n_rows + 7) // 8)
            bound = (64 * tiles + work["reflections"]) // 64 + work["waves"] * (max_bounces + 1)
            print(scene, rows, max_bounces, work, "tiles", tiles, "bound", bound,
                  "occupied lanes per call %.1f" % ((work["pixels"] + work["reflections"]) / work["wave_calls"]))
            assert work["valid"] == 1 and work["pixels"] == w * n_rows
            assert work["reflections"] == int(got["bounces"][band].sum())
            assert 1 <= work["waves"] <= tiles and work["wave_calls"] >= work["waves"]
            assert work["wave_calls"] <= bound
            if max_bounces == 8 and rows == (0, h):
                assert work["reflections"] > 0
            fr.render(rows=rows, max_bounces=max_bounces, count_work=True)
            assert pt.reflection_work() == work  # the same call twice gives the same counts
            quiet = fr.render(rows=rows, max_bounces=max_bounces)  # without the flag: the same bits, and no record
            assert_same({k: quiet[k][band] for k in NAMES}, {k: got[k][band] for k in NAMES}, what="without the flag")
            with pytest.raises(srt.SrtError) as e:
                pt.reflection_work()
            assert e.value.code == srt.capi.ERR_STATE
    finally:
        fr.close()


# ---- 7. the guides reach the denoiser ---------------------------------------------------------------------------------------------
def two_spheres_in_a_mirror(oracle):
    """The camera looks at a large mirror box; a red and a green diffuse sphere stand behind the camera, side by side, so that
    they are seen in the mirror only.  Objects: 0 the mirror, 1 red, 2 green."""
    return [dict(type=oracle.OBJ_BOX, position=(0.0, 0.0, 4.0), half_size=(8.0, 6.0, 1.0), base=(0.9, 0.9, 0.9), specular=(1.0, 1.0, 1.0), **MIRROR),
            dict(type=oracle.OBJ_SPHERE, position=(-1.6, 0.0, -2.0), radius=1.5, base=(0.9, 0.1, 0.1)),
            dict(type=oracle.OBJ_SPHERE, position=(1.6, 0.0, -2.0), radius=1.5, base=(0.1, 0.9, 0.1))], None


RED, GREEN = 1, 2


def test_the_guides_reach_the_denoiser(srt, oracle):
    fr = Frame(srt, oracle, two_spheres_in_a_mirror(oracle), 48, 40)
    try:
        pt = fr.pt
        refl = fr.render()
        obj, J = refl["object"], refl["bounces"]
        red, green = obj == RED, obj == GREEN
        print("red %d pixels (%d through the mirror), green %d" % (red.sum(), (red & (J >= 1)).sum(), green.sum()))
        assert (red & (J >= 1)).sum() >= 20 and green.sum() >= 20
        pt.render(spp=4, bounces=4, seed=1)
        acc = pt.accumulator()
        assert np.isfinite(acc).all()
        poisoned = acc.copy()
        poisoned[green] = np.nan

        # reflection guides: the red sphere's image is isolated from the green one's
        pt.use_reflection_guides(True)
        pt.write_accumulator(poisoned)
        pt.denoise(sigma_color=0.0)
        out = pt.denoised()
        assert np.isfinite(out[red]).all(), "%d red pixels are not finite" % int((~np.isfinite(out[red]).all(axis=-1)).sum())
        assert RR.same_bits(pt.gbuffer("object"), obj)  # the G-buffer slots are the reflection guides now
        with pytest.raises(ValueError):
            pt.temporal()
        # first-hit guides: the mirror is one object, the NaN crosses into the red sphere's image
        pt.use_reflection_guides(False)
        pt.write_accumulator(poisoned)
        pt.denoise(sigma_color=0.0)
        out = pt.denoised()
        first = pt.gbuffer("object")
        assert (first[red & (J >= 1)] == 0).all()  # every one of them is "the mirror" to the first-hit guides
        assert np.isnan(out[red & (J >= 1)]).any()
        assert RR.same_bits(pt.read_reflection("object"), obj)  # the own reflection buffers were not overwritten by the first hits
    finally:
        fr.close()


# ---- the pool refills: a frame with several tiles per wave ------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["Scene3", "Scene1_reflection"])
def test_a_refilling_pool_gives_the_bits_of_one_tile_per_wave(srt, oracle, scene):
    """At 1920 x 1080 there are 32400 tiles, several per wave, so free lanes take pixels of the wave's next tiles while others are
    still on their chains.  A band of eight rows has 240 tiles, at most one per wave — the packing the small frames above
    compare with the CPU reference — and the bands' union must be the whole frame's bits: a pixel's value does not depend on
    how the kernel packs its work."""
    import torch

    w, h = 1920, 1080
    fr = Frame(srt, oracle, SCENES[scene](oracle), w, h, cam=moved_camera(oracle))
    try:
        pt = fr.pt

        def tensors():
            return {k: (torch.full((h, w), -77, dtype=torch.int32, device="cuda:0") if k in ("object", "bounces")
                        else torch.full((h, w, 4), -7.0, dtype=torch.float32, device="cuda:0")) for k in NAMES}

        whole, banded = tensors(), tensors()
        for k in NAMES:
            pt.bind_reflection(k, whole[k])
        pt.render_reflection_gbuffer(count_work=True)
        work = pt.reflection_work()
        tiles = ((w + 7) // 8) * ((h + 7) // 8)
        print(scene, work, "tiles per wave %.1f" % (tiles / work["waves"]), "occupied lanes per call %.1f" % ((work["pixels"] + work["reflections"]) / work["wave_calls"]))
        assert work["pixels"] == w * h and work["reflections"] == int(whole["bounces"].sum().item()) and work["reflections"] > 0
        assert work["waves"] < tiles  # some wave had more than one tile: the pool did refill
        assert work["wave_calls"] <= (64 * tiles + work["reflections"]) // 64 + work["waves"] * 9
        for k in NAMES:
            pt.bind_reflection(k, banded[k])
        for rb in range(0, h, 8):
            pt.render_reflection_gbuffer(rows=(rb, rb + 8))
        pt.wait()
        for k in NAMES:
            assert torch.equal(whole[k].view(torch.int32), banded[k].view(torch.int32)), k
    finally:
        fr.close()


# ---- the host layer and the command line -------------------------------------------------------------------------------------
def scene_json(oracle, objs, path):
    """The scene as a file of the reference's format (Scene.hpp:27-80), for the host layer's loader."""
    import json

    out = []
    for o in objs:
        rend = {"Type": "Sphere", "Radius": o["radius"]} if o["type"] == oracle.OBJ_SPHERE else {"Type": "Cube", "Size": list(o["half_size"])}
        out.append({"Name": "", "Position": list(o["position"]), "Renderer": rend,
                    "Material": {"Color": list(o.get("base", (1, 1, 1))), "Emissive": [0.0, 0.0, 0.0], "Metalness": 0.0,
                                 "Smoothness": o.get("smoothness", 0.5), "SpecularAmount": o.get("specular_amount", 0.0),
                                 "SpecularColor": list(o.get("specular", (1, 1, 1)))}})
    with open(path, "w") as f:
        json.dump({"SceneName": "", "SceneObjects": out}, f)
    return str(path)


def test_host_renderer_and_cli_use_the_reflection_guides(srt, oracle, tmp_path):
    """The isolation check of the test above through PathTraceRenderer::reflectionGuides, then through srt_render.  The command
    line cannot put a NaN into the accumulator, so there the check is that its denoised PPM is, byte for byte, the host layer's
    with the guides on (whose isolation has just been shown), differs from the one with first-hit guides, and that the .npy
    outputs are the C-ABI's reads."""
    import os
    import subprocess

    from conftest import ROOT
    from test_gpu_denoise import _ppm_rgb, tone_map

    w, h = 48, 40
    objs, _ = two_spheres_in_a_mirror(oracle)
    path = scene_json(oracle, objs, tmp_path / "mirror.json")
    # the C-ABI's answer for the scene as the host layer loads it (float32 of the same decimal numbers)
    fr = Frame(srt, oracle, (objs, None), w, h)
    try:
        refl = fr.render()
    finally:
        fr.close()
    red, green, J = refl["object"] == RED, refl["object"] == GREEN, refl["bounces"]

    # PathTraceRenderer::reflectionGuides: the isolation check of the test above through the host layer
    r = srt.host.Renderer(w, h)
    try:
        r.set_scene(srt.host.Scene(path))
        r.settings(fov=55, max_bounces=4, seed=1)
        r.render_reflection_gbuffer(count_work=True)
        for k in NAMES:
            assert RR.same_bits(r.read_reflection(k), refl[k]), k
        assert r.reflection_work()["pixels"] == w * h
        L, ctx = srt.load_library(), r.handle()

        def denoise_poisoned():
            r.render_samples(4)
            acc = r.accumulator()
            acc[green] = np.nan
            assert L.srt_write_accumulator(ctx, acc.ctypes.data_as(C.POINTER(C.c_float))) == 0
            r.denoise(sigma_color=0.0)
            return r.denoised()

        r.reflection_guides(True)
        out = denoise_poisoned()
        assert np.isfinite(out[red]).all()
        assert RR.same_bits(r.gbuffer("object"), refl["object"])  # render_gbuffer rendered the reflection guides
        r.render_temporal_frame(2, False)  # the temporal pass keeps first hits, and the binding comes back afterwards
        assert (r.gbuffer("object")[red] == RED).all()
        r.invalidate()
        r.reflection_guides(False)
        out = denoise_poisoned()
        assert (r.gbuffer("object")[red & (J >= 1)] == 0).all() and np.isnan(out[red & (J >= 1)]).any()
    finally:
        r.close()

    # srt_render --denoise --reflection-guides --reflection-out
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    base = [cli, "--scene", path, "--width", str(w), "--height", str(h), "--spp", "4", "--bounces", "4", "--seed", "1"]
    run = lambda extra: subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
    r1 = run(["--out", str(tmp_path / "a.ppm"), "--denoise", str(tmp_path / "first.ppm")])
    r2 = run(["--out", str(tmp_path / "b.ppm"), "--denoise", str(tmp_path / "refl.ppm"), "--reflection-guides", "--reflection-out", str(tmp_path / "g")])
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr[-1000:] + r2.stderr[-1000:]
    assert (tmp_path / "a.ppm").read_bytes() == (tmp_path / "b.ppm").read_bytes()
    for k in NAMES:  # rows top-down like the PPM
        assert RR.same_bits(np.load(tmp_path / ("g_%s.npy" % k))[::-1], refl[k]), k
    hr = srt.host.Renderer(w, h)
    try:
        hr.set_scene(srt.host.Scene(path))
        hr.settings(fov=55, max_bounces=4, seed=1)
        want = {}
        for name, on in (("first", False), ("refl", True)):
            hr.invalidate()
            hr.render_samples(4, count_rays=True)
            hr.reflection_guides(on)
            hr.denoise()
            px = tone_map(hr.denoised())[::-1]
            want[name] = np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], -1).astype(np.uint8)
    finally:
        hr.close()
    first, with_guides = _ppm_rgb(tmp_path / "first.ppm", w, h), _ppm_rgb(tmp_path / "refl.ppm", w, h)
    assert np.array_equal(first, want["first"]) and np.array_equal(with_guides, want["refl"])
    assert not np.array_equal(first, with_guides)  # the guides do change what the filter does to the mirror
    # fewer reflections: the mirror is a first hit again
    r3 = run(["--out", str(tmp_path / "c.ppm"), "--denoise", str(tmp_path / "zero.ppm"), "--reflection-guides", "--reflection-bounces", "0",
              "--reflection-out", str(tmp_path / "z")])
    assert r3.returncode == 0, r3.stderr[-1000:]
    assert np.array_equal(_ppm_rgb(tmp_path / "zero.ppm", w, h), first) and not np.load(tmp_path / "z_bounces.npy").any()
