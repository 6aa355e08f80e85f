"""srt_render's refusals, replayed from tests/golden/cli_refusals.json (made by tests/golden/make_cli_refusals.py from the
front end as it stood before host/srt_cli.cpp got its option table): for every recorded command line the exit status and the
whole of stderr are what they were — the texts, the usage text byte for byte, and which message wins when several rules are
broken — nothing goes to stdout and no output file appears.  Every command ends before a renderer is created, so no GPU is
needed."""
import importlib.util
import json
import os
import shlex

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
GOLDEN = os.path.join(ROOT, "tests", "golden")

_spec = importlib.util.spec_from_file_location("make_cli_refusals", os.path.join(GOLDEN, "make_cli_refusals.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def record():
    with open(gen.RECORD) as f:
        return json.load(f)


def test_the_record_holds_the_generators_cases(record):
    cases = record["cases"]
    assert [shlex.split(e["argv"]) for e in cases] == gen.cases()
    assert all(e["status"] in (1, 2) and e["outputs"] == [] and "srt_create" not in e["stderr"] for e in cases)
    # what the list has to reach: every option without its value, the usage text, the parsers' messages and the ordered pairs
    stderr = {e["stderr"] for e in cases}
    for name in gen.VALUE_OPTIONS:
        assert name + " needs a value\n" in stderr, name
    assert record["usage"].startswith("usage: srt_render --scene FILE") and len(record["usage"]) > 10000
    assert sum(e["stderr"] == "{USAGE}" for e in cases) >= 10
    assert {"--move wants R,U,F\n", "--move-object wants IDX:DX,DY,DZ\n"} <= stderr
    assert len(stderr) >= 110  # the ~35 rule messages, the 60 missing values, the parsers', the files' and the scene's


def test_srt_render_refuses_as_recorded(record, tmp_path):
    tmp = str(tmp_path)
    gen.make_inputs(tmp)
    for want in record["cases"]:
        got, stdout = gen.run_case(CLI, shlex.split(want["argv"]), tmp, record["usage"])
        assert got == want, (want, got)
        assert stdout == "" and got["outputs"] == [], (want["argv"], stdout, got["outputs"])
