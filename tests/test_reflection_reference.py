"""The Python restatement of the reflection guides' definition (tests/reflection_reference.py) on the CPU: it reduces to the
oracle's first hits where nothing reflects, it finds the chains the shipped scenes are known to have (so that the GPU comparison
in tests/test_gpu_reflection.py is not vacuous), and it gives hand-made known answers."""
import numpy as np

import reflection_reference as RR
import visibility_reference as VR
from conftest import scene_path

F = np.float32
W, H = 24, 20

# pixels of the 24 x 20 frame (default camera, defaults) by number of reflections J: (chain ends on an object, chain leaves the scene)
COUNTS = {
    "Scene1_reflection": ({0: 82, 1: 48, 2: 10, 3: 6, 8: 2}, {0: 185, 1: 101, 2: 16, 3: 10, 4: 7, 5: 6, 6: 2, 7: 3, 8: 2}),
    "Scene3": ({0: 20, 1: 207}, {0: 23, 1: 230}),
    "Scene_indirect": ({0: 363, 1: 89, 2: 5}, {0: 23}),
    "Scene1": ({0: 295}, {0: 185}),
}


def frame(oracle, name):
    oarr, n = oracle.make_objects(oracle.load_scene_json_py(scene_path(name)))
    return oarr, n, RR.reference(oracle, oarr, n, oracle.default_camera(), W, H)


def test_scene1_reflects_nothing_and_equals_the_first_hits(oracle):
    oarr, n, ref = frame(oracle, "Scene1")
    assert RR.histogram(ref) == COUNTS["Scene1"]
    assert not ref["bounces"].any()
    obj, nd, pos = VR.oracle_gbuffer(oracle, oarr, n, oracle.default_camera(), W, H)
    assert RR.same_bits(ref["object"], obj) and RR.same_bits(ref["normal_depth"], nd) and RR.same_bits(ref["position"], pos)
    for y in range(H):
        for x in range(W):
            i = obj[y, x]
            want = [0.0] * 4 if i < 0 else [RR.c0(v) for v in oarr[i].material.base_color] + [0.0]
            assert RR.same_bits(ref["albedo"][y, x], np.array(want, F))


def test_shipped_scenes_have_the_chains_the_gpu_comparison_needs(oracle):
    for name in ("Scene1_reflection", "Scene3", "Scene_indirect"):
        _, _, ref = frame(oracle, name)
        on, off = RR.histogram(ref)
        print(name, on, off)
        if name == "Scene1_reflection":
            assert all(on.get(J, 0) > 0 for J in (0, 1, 2, 3, 8)) and all(off.get(J, 0) > 0 for J in range(9))
        assert (on, off) == COUNTS[name]
        # a chain that leaves the scene has the miss values, one that ends on an object a finite path length
        left = ref["object"] == -1
        assert np.isposinf(ref["normal_depth"][left][:, 3]).all() and not ref["position"][left].any() and not ref["albedo"][left].any()
        assert np.isfinite(ref["normal_depth"][~left][:, 3]).all() and (ref["position"][~left][:, 3] == 1).all()


A = dict(base=(0.9, 0.8, 0.7), specular=(0.11, 0.12, 0.13))
B = dict(base=(0.6, 0.5, 0.4), specular=(0.95, 0.85, 0.75))
S = (0.3, 0.2, 0.1)


# a ray at 45 degrees to the y axis with no zero component (a box is missed by a ray with one): d = (1, -sqrt 2, 1) / 2
O = (F(-1.0), F(0.0), F(4.0))
R2 = 2 ** 0.5
P0 = (-1 + R2 / 2, -1.0, 4 + R2 / 2)  # where it meets y = -1, at distance sqrt 2


def ray():
    return RR.normalized((F(1.0), F(-R2), F(1.0)))


def along(p, d, t):
    return tuple(a + b * t for a, b in zip(p, d))


def mirror_floor(oracle):
    return dict(type=oracle.OBJ_BOX, position=(0.0, -1.5, 5.0), half_size=(3.0, 0.5, 3.0), smoothness=1.0, specular_amount=1.0, **A)


def test_known_answer_one_mirror(oracle):
    """A ray at 45 degrees onto the top face (y = -1) of an axis-aligned mirror box leaves as (d.x, -d.y, d.z) and meets a diffuse
    sphere on that line: J = 1, albedo = base_box * base_sphere per channel."""
    objs = [mirror_floor(oracle), dict(type=oracle.OBJ_SPHERE, position=along(P0, (0.5, R2 / 2, 0.5), 3.0), radius=0.5, base=S)]
    oarr, n = oracle.make_objects(objs)
    trace = RR.Tracer(oracle, oarr, n)
    d, o = ray(), O
    i0, n0, p0, t0 = trace(o, d)
    assert i0 == 0 and [float(v) for v in n0] == [0.0, 1.0, 0.0] and abs(float(t0) - 2 ** 0.5) < 1e-6
    r = RR.normalized(RR.reflect(d, n0))
    assert all(abs(float(a) - float(b)) <= 2.0 ** -23 for a, b in zip(r, (d[0], -d[1], d[2])))
    i, nd, pos, alb, J = RR.chain(trace, oarr, o, d)
    assert (i, J) == (1, 1)
    i1, n1, p1, t1 = trace(RR.offset(p0, n0), r)
    assert i1 == 1 and nd[3] == F(t0 + t1) and nd[:3] == n1 and pos == (p1[0], p1[1], p1[2], F(1.0))
    assert alb == tuple(F(F(a) * F(s)) for a, s in zip(A["base"], S)) + (F(0.0),)
    # nothing is followed with max_bounces = 0 or +inf thresholds: the first hit
    for kw in (dict(max_bounces=0), dict(min_smoothness=np.inf), dict(min_specular=np.inf)):
        i, nd, pos, alb, J = RR.chain(trace, oarr, o, d, **kw)
        assert (i, J) == (0, 0) and nd == (n0[0], n0[1], n0[2], t0) and alb == tuple(F(v) for v in A["base"]) + (F(0.0),)
    # ... and a NaN material fails the comparison
    oarr[0].material.smoothness = float("nan")
    assert RR.chain(trace, oarr, o, d)[4] == 0


def test_known_answer_two_mirrors(oracle):
    """With a second mirror box overhead the chain has J = 2: the base colour of the first surface, the specular colour of the
    mirror at hit 1 (every mirror after the first enters through Lerp(base, specular, 1)), the dissipation 0.8f of the second
    bounce, then the terminal's base colour — in that order."""
    objs = [mirror_floor(oracle),
            dict(type=oracle.OBJ_BOX, position=(0.0, 2.5, 8.0), half_size=(3.0, 0.5, 3.0), smoothness=1.0, specular_amount=1.0, **B),
            dict(type=oracle.OBJ_SPHERE, position=along(along(P0, (0.5, R2 / 2, 0.5), 3 * R2), (0.5, -R2 / 2, 0.5), 3.0), radius=0.5, base=S)]
    oarr, n = oracle.make_objects(objs)
    trace = RR.Tracer(oracle, oarr, n)
    d = ray()
    i, nd, pos, alb, J = RR.chain(trace, oarr, O, d)
    assert (i, J) == (2, 2)
    want = tuple(F(F(F(F(a) * F(b)) * F(0.8)) * F(s)) for a, b, s in zip(A["base"], B["specular"], S))
    assert alb == want + (F(0.0),)
    assert want != tuple(F(F(F(F(a) * F(0.8)) * F(b)) * F(s)) for a, b, s in zip(A["base"], B["specular"], S))  # the order shows
    # one reflection allowed: the chain ends on the second mirror with its BASE colour
    i, nd, pos, alb, J = RR.chain(trace, oarr, O, d, max_bounces=1)
    assert (i, J) == (1, 1) and alb == tuple(F(F(a) * F(b)) for a, b in zip(A["base"], B["base"])) + (F(0.0),)
