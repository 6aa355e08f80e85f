"""What classification buys, asserted: tools/probe_states_quality.py's protocol at 96 x 54 and grid spacing 0.5, where 789 of the 1287
probes lie inside objects.  One measured run gave rmse(depth) / rmse(depth + classification) = 19.2 (Scene_indirect: 0.9716 /
0.0505) and 17.8 (closed room: 1.0144 / 0.0570); the test asserts a ratio of 2.  The reference is a 4096-sample srt_render of the
same frame; the error is the relative luminance RMSE over the diffuse hit pixels."""
import os
import sys

import numpy as np
import pytest

import probe_grid_reference as PG
from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

W, H = 96, 54


@pytest.mark.parametrize("name", ["Scene_indirect", "closed_room"])
def test_classification_at_least_halves_the_error_of_the_filtered_call_at_spacing_half(srt, name):
    from probe_grid_quality import lum
    from probe_grid_time import bounds_grid

    scene = srt.host.Scene(scene_path("Scene_indirect"))
    if name == "closed_room":
        wall = srt.Object()
        wall.type, wall.position[:], wall.half_size[:] = 2, (0.0, 0.0, -0.3), (6.0, 6.0, 0.2)
        wall.material.base_color[:] = (0.5, 0.5, 0.5)
        scene.add(wall, "wall behind the camera")
    objs, cnt = scene.objects_copy()
    diffuse = np.array([objs[i].material.specular_amount == 0.0 for i in range(cnt)])
    emissive = np.array([list(objs[i].material.emissive_color) for i in range(cnt)], np.float64)
    pt = srt.PathTracer(W, H)
    try:
        pt.set_scene(objs, cnt)
        pt.set_camera(srt.default_camera())
        for first in range(1, 4097, 256):
            pt.render(spp=256, bounces=8, seed=2, first_sample=first, reset=(first == 1))
        ref = lum(pt.accumulator())
        pt.render_gbuffer()
        obj, pos = pt.gbuffer("object"), pt.gbuffer("position")
        mask = (obj != -1) & diffuse[np.maximum(obj, 0)]
        glow = lum(emissive[np.maximum(obj, 0)])

        def rmse():
            e = (lum(pt.probe_grid_output())[mask] + glow[mask] - ref[mask]) / (ref[mask] + 0.01)
            return float(np.sqrt(np.mean(e * e)))

        grid = bounds_grid(obj, pos, 0.5)
        pt.trace_light_probes(srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts), 256, samples=16, bounces=8, seed=3)
        coeff = pt.light_probe_coefficients()
        pt.trace_probe_depth(resolution=16, sharpness=5, max_distance=1.5 * float(np.sqrt(3.0)) * 0.5)
        depth = pt.probe_depth_output("moments")
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.classify_probes(count_work=True)
        rec, work = pt.probe_states_output("records"), pt.probe_states_work()
        kw = dict(albedo=True, band_weight=PG.HEMISPHERE)
        pt.shade_probe_grid_depth(coefficients=coeff, moments=depth, resolution=16, **kw)
        plain = rmse()
        pt.shade_probe_grid_states(states=rec, depth=True, **kw)
        classified = rmse()
        print("%s: %d of %d probes inside; rmse depth %.4f, depth + classification %.4f, ratio %.1f" % (name, work["inside"], work["probes"], plain, classified,
                                                                                                     plain / classified))
        assert work["inside"] > work["probes"] // 2
        assert plain >= 2.0 * classified
    finally:
        pt.close()
