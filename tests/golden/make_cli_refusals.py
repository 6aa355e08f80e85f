#!/usr/bin/env python3
"""Generates tests/golden/cli_refusals.json: what srt_render says when it refuses a command line.

What this fixture is: a REGRESSION pin of the command-line front end (host/srt_cli.cpp) — for a list of argument vectors that
srt_render refuses before it creates a renderer (so no GPU is needed), the exit status, the whole of stderr and the output
files that exist afterwards (none).  The messages, and which one wins when two rules are broken, are what users and scripts
see; tests/test_cli_refusals.py replays the record against the tree's srt_render.
What it is NOT: a specification.  The record is made from an srt_render built from the commit BEFORE a change to the front end
(never from the tree under test) and committed unedited.

    python tests/golden/make_cli_refusals.py --cli PATH/TO/srt_render            # writes the record
    python tests/golden/make_cli_refusals.py --cli PATH/TO/srt_render --check    # compares instead, exit status 1 on a difference

The scene path and the scratch directory are written as the placeholders {SCENE} and {TMP}; the usage text, which a
dozen of the cases print whole, is kept once ("usage") and written as {USAGE} in their stderr.
"""
import argparse
import json
import os
import shlex
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
RECORD = os.path.join(HERE, "cli_refusals.json")
SCENE = os.path.join(ROOT, "software-raytracer_amd", "scenes", "Scene1.json")

# every option that takes a value (given last without one: "--x needs a value")
VALUE_OPTIONS = """--scene --width --height --spp --bounces --fov --seed --device --devices --out --resave --gbuffer --denoise
--denoise-variance --steps --upsample --aa --rays --rays-out --radiance --probes --probes-out --probe-directions
--probe-radiance-out --probe-grid --irradiance-out --probe-depth --probe-depth-sharpness --probe-depth-max --probe-depth-bias
--probe-depth-out --probe-clearance --probe-max-offset --probe-steps --states-out --probe-update --probe-hysteresis
--probe-tail-grid --probe-tail-coefficients --probe-feedback --probe-cascade --probe-cascade-blend --probe-scroll
--probe-scroll-after --probe-bounces --probe-samples --adaptive --adaptive-threshold --adaptive-max --counts-out --ao
--ao-radius --vis-out --mirror-radius --reflection-bounces --reflection-out --temporal --turn --move --move-object""".split()

# the input files of the scratch directory: name -> number of float32 (zeros)
INPUTS = {"rays.f32": 8, "rays7.f32": 7, "empty.f32": 0, "probes.f32": 4, "probes5.f32": 5, "dirs.f32": 8, "dirs6.f32": 6,
          "dirs4097.f32": 4 * 4097, "coeff8.f32": 8 * 36, "coeff7.f32": 7 * 36}

S = ["--scene", "{SCENE}"]
T = "{TMP}/"
GRID = "0,0,0,1,1,1,2,2,2"  # 8 probes
OUT = ["--irradiance-out", T + "irr.bin"]
IO = S + ["--probe-grid", GRID, "--probe-directions", "16"] + OUT
RAYS = S + ["--rays", T + "rays.f32", "--rays-out", T + "rays.bin"]
PROBES = S + ["--probes", T + "probes.f32", "--probe-directions", "16", "--probes-out", T + "probes.bin"]
CLASSIFY = IO + ["--probe-classify"]
TAIL = IO + ["--probe-tail"]
RAYTAIL = RAYS + ["--radiance", "2", "--probe-tail", "--probe-tail-grid", GRID, "--probe-tail-coefficients"]
VIS = S + ["--sun-visibility", "--vis-out", T + "vis.bin"]
DV = S + ["--denoise-variance", T + "dv.ppm"]
# the twelve frame options that --probe-grid and --probes refuse; --rays refuses the first six, --adaptive five of them
FRAME_OPTIONS = [["--steps", "2"], ["--aa", "2"], ["--gbuffer", T + "g"], ["--denoise", T + "d.ppm"], ["--upsample", T + "u.ppm"],
                 ["--denoise-variance", T + "dv.ppm"], ["--adaptive", "1"], ["--ao", "4"], ["--sun-visibility"], ["--vis-out", T + "vis.bin"],
                 ["--reflection-guides"], ["--reflection-out", T + "r"]]


def with_grid(text):
    return S + ["--probe-grid", text, "--probe-directions", "16"] + OUT


def cases():
    c = []
    # --- options and their values
    c += [[], ["--bogus"], S + ["--bogus"], S + ["scene.json"], ["--move", "bad", "--bogus"], ["--bogus", "--move", "bad"]]
    c += [(S if name != "--scene" else []) + [name] for name in VALUE_OPTIONS]
    c += [S + [name, "abc"] for name in ("--width", "--height", "--spp", "--steps", "--aa")] + [S + ["--temporal", "-1"], S + ["--width", "0"], S + ["--height", "-1"],
                                                                                               S + ["--spp", "0"], S + ["--steps", "0"], ["--width", "64"]]
    # --- the hand-written parsers (refused while parsing, before any rule: the --refit of the last ones is never looked at)
    c += [S + ["--move", v] for v in ("1,2", "1,2,3,4", "a,b,c")] + [["--refit", "--move", "1"]]
    c += [S + ["--move-object", v] for v in ("0", "0:1,2", "x:1,2,3", "0:1,2,3,4")] + [["--refit", "--move-object", "1"]]
    c += [TAIL + ["--probe-feedback", "3", "--probe-scroll", v] for v in ("1,2", "1,2,3,4", "1,x,3", "1.5,2,3")]
    c += [with_grid(g) for g in ("1,2,3", "0,0,0,1,1,1,2,2,x", "0,0,0,1,1,1,2,2,2,2", "0,0,0,1,1,1,0,2,2", "0,0,0,0,1,1,2,2,2",
                                 "0,nan,0,1,1,1,2,2,2", "0,0,0,1,1,1,65536,65536,2", "0,0,0,1,1,1,1024,1024,2048")]
    c += [RAYTAIL[:-3] + ["--probe-tail-grid", g, "--probe-tail-coefficients", T + "coeff8.f32"] for g in ("1,2,3", "0,0,0,1,1,0,2,2,2")]
    # --- the rules, in their order
    c += [S + ["--move-object", "0:1,0,0"], S + ["--refit"], S + ["--temporal", "2", "--refit"]]
    c += [S + ["--rays", T + "rays.f32"], S + ["--rays-out", T + "rays.bin"], S + ["--rays-normalize"], S + ["--any-hit"]]
    c += [S + ["--probe-depth", "8"], IO + ["--probe-depth-bias", "0.1"], IO + ["--probe-depth-out", T + "m.bin"], IO + ["--probe-depth", "8", "--probe-visibility"]]
    c += [IO + ["--probe-depth", "5"], IO + ["--probe-depth", "x"]] + [IO + ["--probe-depth", "8"] + e for e in (
        ["--probe-depth-sharpness", "7"], ["--probe-depth-sharpness", "-1"], ["--probe-depth-max", "0"], ["--probe-depth-max", "inf"], ["--probe-depth-bias", "-1"],
        ["--probe-depth-bias", "inf"])]
    c += [S + ["--probe-classify"], IO + ["--probe-relocate"], IO + ["--states-out", T + "s.bin"], CLASSIFY + ["--probe-visibility"]]
    c += [CLASSIFY + e for e in (["--probe-clearance", "0"], ["--probe-clearance", "0.6"], ["--probe-max-offset", "0"],
                                 ["--probe-max-offset", "0.51"], ["--probe-steps", "0"], ["--probe-steps", "65"])]
    c += [S + ["--probe-update", "2"], IO + ["--probe-update", "2"], CLASSIFY + ["--probe-hysteresis", "0.5"], CLASSIFY + ["--probe-samples", "2"]]
    c += [CLASSIFY + ["--probe-update"] + e for e in (["0"], ["4097"], ["2", "--probe-samples", "0"], ["2", "--probe-samples", "4097"], ["2", "--probe-hysteresis", "1"],
                                                      ["2", "--probe-hysteresis", "-0.1"])]
    c += [IO + ["--probe-tail-frame"], S + ["--probe-tail", "--probe-tail-frame"]]
    c += [TAIL + ["--probe-tail-frame"] + e for e in (["--devices", "0"], ["--temporal", "2"], ["--adaptive", "1"], ["--steps", "2"])]
    c += [S + ["--probe-cascade", "2"], IO + ["--probe-cascade-blend", "2"]] + [IO + ["--probe-cascade"] + e for e in (
        ["0"], ["5"], ["2", "--probe-cascade-blend", "0"], ["2", "--probe-cascade-blend", "inf"], ["2", "--probe-visibility"],
        ["2", "--probe-tail"], ["2", "--probe-classify", "--probe-update", "2"],
        ["2", "--temporal", "2", "--move-object", "0:1,0,0"], ["2", "--probe-depth", "8", "--probe-depth-out", T + "m.bin"], ["2", "--probe-classify", "--states-out", T + "s.bin"])]
    c += [S + ["--probe-scroll", "1,0,0"], S + ["--probe-scroll-after", "1"], TAIL + ["--probe-scroll", "1,0,0"], TAIL + ["--probe-feedback", "3", "--probe-scroll-after", "2"]]
    c += [TAIL + ["--probe-feedback", "3", "--probe-scroll", "1,0,0", "--probe-scroll-after", v] for v in ("0", "4", "x")]
    c += [TAIL + ["--probe-tail-grid", GRID], TAIL + ["--probe-tail-coefficients", T + "coeff8.f32"], CLASSIFY + ["--probe-update", "2", "--probe-tail"]]
    c += [TAIL + ["--probe-feedback", "0"], TAIL + ["--probe-feedback", "4097"], TAIL + ["--probe-bounces", "-1"], IO + ["--probe-feedback", "0"], IO + ["--probe-bounces", "-1"]]
    c += [TAIL + ["--probe-tail-depth"], TAIL + ["--probe-tail-states"], IO + ["--probe-tail-depth"], TAIL + ["--probe-depth", "8", "--probe-tail-depth", "--probe-tail-states"]]
    c += [S + e for e in (["--probe-tail"], ["--probe-tail-depth"], ["--probe-tail-states"], ["--probe-tail-normal-weight"], ["--probe-feedback", "2"], ["--probe-bounces", "1"],
                          ["--probe-tail-grid", GRID], ["--probe-tail-coefficients", T + "coeff8.f32"])]
    c += [RAYS + ["--probe-tail", "--probe-tail-grid", GRID, "--probe-tail-coefficients", T + "coeff8.f32"], RAYTAIL[:-1], RAYTAIL[:-3] + RAYTAIL[-1:] + [T + "coeff8.f32"],
          RAYTAIL + [T + "coeff8.f32", "--probe-tail-depth"], RAYTAIL + [T + "coeff8.f32", "--probe-tail-states"], RAYTAIL + [T + "coeff8.f32", "--probe-feedback", "2"],
          RAYTAIL + [T + "coeff8.f32", "--probe-bounces", "1"], [a for a in RAYTAIL if a != "--probe-tail"] + [T + "coeff8.f32"],
          PROBES + ["--radiance", "2", "--probe-tail", "--probe-tail-grid", GRID, "--probe-tail-coefficients", T + "coeff8.f32"]]
    c += [S + OUT] + [S + [f] for f in ("--probe-visibility", "--probe-normal-weight", "--probe-albedo", "--probe-hemisphere")] + [S + OUT + ["--probe-directions", "16"]]
    c += [IO[:-2], IO + RAYS[2:], IO + PROBES[2:4] + PROBES[6:], IO + ["--probes-out", T + "probes.bin"], IO + ["--probe-radiance-out", T + "pr.bin"], IO + ["--temporal", "2"],
          IO + ["--devices", "0"], IO + ["--devices", "0", "--temporal", "2"] + RAYS[2:]]
    c += [S + ["--probe-grid", GRID] + OUT] + [S + ["--probe-grid", GRID, "--probe-directions", k] + OUT for k in ("0", "4097", "dirs.f32", "-1", "99999999999")]
    c += [IO + e for e in (["--radiance", "0"], ["--radiance", "4097"], ["--bounces", "-1"])] + [IO + e for e in FRAME_OPTIONS]
    c += [S + ["--radiance", "4"], RAYS + ["--any-hit", "--radiance", "4"], RAYS + ["--radiance", "0"], RAYS + ["--radiance", "4097"], RAYS + ["--radiance", "4", "--bounces", "-1"]]
    c += [S + ["--probes", T + "probes.f32"], S + ["--probes-out", T + "probes.bin"], S + ["--probe-directions", "16"], S + ["--probe-radiance-out", T + "pr.bin"],
          PROBES[:4] + PROBES[6:], PROBES[:2] + PROBES[4:], PROBES[:6]]
    c += [PROBES + e for e in (["--radiance", "0"], ["--radiance", "4097"], ["--bounces", "-1"], RAYS[2:], ["--devices", "0"], ["--temporal", "2"])] + [PROBES + e for e in FRAME_OPTIONS]
    c += [RAYS + e for e in (["--devices", "0"], ["--temporal", "2"])] + [RAYS + e for e in FRAME_OPTIONS[:6]]
    c += [S + ["--ao", "4"], S + ["--sun-visibility"], S + ["--vis-out", T + "vis.bin"], S + ["--ao-radius", "1"], VIS + ["--ao-radius", "1"]]
    c += [S + ["--vis-out", T + "vis.bin", "--ao"] + e for e in (["0"], ["4097"], ["x"], ["4", "--ao-radius", "0"], ["4", "--ao-radius", "nan"])]
    c += [VIS + ["--devices", "0"], VIS + ["--temporal", "2"], RAYS + VIS[2:], RAYS + ["--ao", "4"]]
    c += [S + ["--reflection-guides"], S + ["--reflection-bounces", "4"], RAYS + ["--reflection-guides"]] + [S + ["--reflection-out", T + "r"] + e for e in (
        ["--reflection-bounces", "-1"], ["--reflection-bounces", "65"], ["--devices", "0"], ["--temporal", "2"], ["--adaptive", "1"], RAYS[2:])]
    c += [S + ["--mirror-history"], S + ["--mirror-radius", "2"], S + ["--temporal", "2", "--mirror-radius", "2"], S + ["--temporal", "2", "--mirror-history", "--mirror-radius", "0"],
          S + ["--temporal", "2", "--mirror-history", "--mirror-radius", "x"]]
    c += [S + ["--temporal-variance"]] + [S + ["--temporal", "2", "--temporal-variance"] + e for e in (["--devices", "0"], ["--steps", "2"], ["--upsample", T + "u.ppm"])]
    c += [S + ["--denoise", T + "d.ppm", "--devices", "0"], S + ["--steps", "2", "--devices", "0"], S + ["--upsample", T + "u.ppm", "--devices", "0"],
          S + ["--steps", "2", "--temporal", "2"], S + ["--upsample", T + "u.ppm", "--temporal", "2"]]
    c += [DV + e for e in (["--denoise", T + "d.ppm"], ["--spp", "3"], ["--spp", "1"], ["--devices", "0"], ["--temporal", "2"], ["--steps", "2"], ["--upsample", T + "u.ppm"])]
    c += [S + ["--adaptive-threshold", "0.1"], S + ["--adaptive-max", "8"], S + ["--counts-out", T + "c.bin"]]
    c += [S + ["--adaptive"] + e for e in (["0"], ["65"], ["x"], ["2", "--spp", "3"], ["2", "--spp", "1"], ["2", "--bounces", "-1"], ["2", "--adaptive-threshold", "0"],
                                           ["2", "--adaptive-max", "0"], ["2", "--adaptive-max", "4097"])]
    c += [S + ["--adaptive", "2"] + e for e in [["--devices", "0"], ["--temporal", "2"], RAYS[2:], VIS[2:], ["--ao", "4", "--vis-out", T + "vis.bin"]] + FRAME_OPTIONS[:2] + FRAME_OPTIONS[3:6]]
    c += [S + ["--aa", "0"], S + ["--aa", "5"], S + ["--aa", "2", "--devices", "0"], S + ["--temporal", "2", "--devices", "0"], S + ["--temporal", "2", "--devices", "0,1", "--equal-bands"]]
    # --- two rules broken at once: the first in the order above wins
    c += [["--refit"], ["--move-object", "0:1,0,0"], ["--rays", T + "rays.f32"], S + ["--rays", T + "rays.f32", "--probe-depth", "8"],
          CLASSIFY + ["--probe-depth", "8", "--probe-visibility"], CLASSIFY + ["--probe-depth", "5", "--probe-steps", "0"],
          IO + ["--probe-steps", "0", "--probe-update", "0"], TAIL + ["--probe-tail-frame", "--steps", "2", "--probe-cascade", "2"], IO + ["--probe-cascade", "0", "--probe-scroll", "1,0,0"],
          TAIL + ["--probe-scroll", "1,0,0", "--probe-tail-grid", GRID], with_grid("1,2,3") + ["--probe-tail", "--probe-tail-grid", GRID],
          with_grid("1,2,3") + ["--probe-tail", "--probe-feedback", "0"], IO[:-2] + ["--devices", "0"],
          S + ["--probe-grid", GRID, "--probe-directions", "0", "--radiance", "0"] + OUT, IO + ["--radiance", "0", "--ao", "4"],
          S + ["--radiance", "4", "--probes-out", T + "probes.bin"], PROBES + ["--radiance", "0", "--gbuffer", T + "g"],
          RAYS + ["--denoise", T + "d.ppm", "--devices", "0"], RAYS + ["--sun-visibility", "--reflection-out", T + "r"],
          S + ["--ao", "4", "--reflection-guides"], S + ["--mirror-history", "--temporal-variance"],
          S + ["--temporal-variance", "--denoise", T + "d.ppm", "--devices", "0"],
          DV + ["--denoise", T + "d.ppm", "--devices", "0"], DV + ["--spp", "3", "--adaptive-max", "8"],
          S + ["--adaptive", "0", "--aa", "5"], S + ["--adaptive", "2", "--reflection-out", T + "r"],
          S + ["--aa", "5", "--temporal", "2", "--devices", "0"]]
    # --- refused after the scene is loaded, before a renderer is created
    c += [S + ["--temporal", "2", "--move-object", "99:1,0,0"], S + ["--temporal", "2", "--move-object", "0:1,0,0", "--move-object", "4000000000:1,0,0"],
          CLASSIFY + ["--probe-update", "2", "--move-object", "99:1,0,0"]]
    c += [S + ["--rays", T + name, "--rays-out", T + "rays.bin"] for name in ("rays7.f32", "empty.f32", "missing.f32")]
    c += [S + ["--probes", T + name, "--probe-directions", "16", "--probes-out", T + "probes.bin"] for name in ("probes5.f32", "empty.f32", "missing.f32")]
    c += [PROBES[:4] + ["--probe-directions", k] + PROBES[6:] for k in ("0", "5000", T + "dirs4097.f32", T + "dirs6.f32", T + "missing.f32")]
    c += [S + ["--probes", T + "probes5.f32", "--probe-directions", "0", "--probes-out", T + "probes.bin"]]
    c += [RAYTAIL + [T + name] for name in ("coeff7.f32", "probes5.f32", "missing.f32")]
    c += [RAYS[:2] + ["--rays", T + "rays7.f32", "--rays-out", T + "rays.bin"] + RAYTAIL[6:] + [T + "coeff7.f32"], RAYS[:2] + ["--rays", T + "rays7.f32", "--rays-out", T + "rays.bin"] + RAYTAIL[6:] + [T + "coeff8.f32"]]
    return c


def make_inputs(tmp):
    for name, n in INPUTS.items():
        with open(os.path.join(tmp, name), "wb") as f:
            f.write(struct.pack("<%df" % n, *([0.0] * n)))


def run_case(cli, argv, tmp, usage):
    """One command: its exit status, stdout, stderr and the files it left in tmp.  In stderr the paths are written back as
    placeholders, and so is the usage text `usage` ({USAGE}: the record holds its bytes once, not once per case)."""
    real = [a.replace("{SCENE}", SCENE).replace("{TMP}", tmp) for a in argv]  # (argv: a list)
    r = subprocess.run([cli] + real, capture_output=True, text=True, timeout=60, cwd=tmp)
    left = sorted(set(os.listdir(tmp)) - set(INPUTS))
    stderr = r.stderr.replace(usage, "{USAGE}").replace(SCENE, "{SCENE}").replace(tmp, "{TMP}")
    return {"argv": shlex.join(argv), "status": r.returncode, "stderr": stderr, "outputs": left}, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli", required=True, help="the srt_render to record (the parent commit's) or, with --check, to compare")
    ap.add_argument("--check", action="store_true", help="compare with the record instead of writing it")
    a = ap.parse_args()
    cli = os.path.abspath(a.cli)
    if a.check:
        with open(RECORD) as f:
            record = json.load(f)
        usage, want = record["usage"], record["cases"]
    else:  # the usage text is what the recorded binary prints when it is given nothing
        usage = subprocess.run([cli], capture_output=True, text=True, timeout=60).stderr
        assert usage.startswith("usage: srt_render --scene FILE"), usage[:200]
    with tempfile.TemporaryDirectory() as tmp:
        make_inputs(tmp)
        got = []
        for argv in cases():
            entry, stdout = run_case(cli, argv, tmp, usage)  # ("argv" of the entry: one shell-quoted string)
            assert stdout == "" and not entry["outputs"] and entry["status"] in (1, 2), ("not a refusal", entry, stdout)
            assert "srt_create" not in entry["stderr"], ("reached the renderer", entry)
            got.append(entry)
    if a.check:
        bad = [(w, g) for w, g in zip(want, got) if w != g]
        for w, g in bad:
            print("DIFFERS\n  recorded %r\n  got      %r" % (w, g))
        print("%d cases, %d differ%s" % (len(got), len(bad), "" if len(want) == len(got) else "; the record holds %d" % len(want)))
        sys.exit(1 if bad or len(want) != len(got) else 0)
    note = "srt_render's refusals as the commit before the change gave them; made by make_cli_refusals.py, not edited"
    with open(RECORD, "w") as f:  # one case per line
        f.write('{"note": %s,\n"usage": %s,\n"cases": [\n%s\n]}\n' % (json.dumps(note), json.dumps(usage), ",\n".join(json.dumps(e, separators=(",", ":")) for e in got)))
    print("%d cases -> %s" % (len(got), RECORD))


if __name__ == "__main__":
    main()
