"""CPU: the environment switches of libgpx.so have ONE definition (csrc/gpx_env.h) and the documented table is its copy.

gpx_debug_env (no device needed) prints a fresh snapshot of every switch, one NAME=value line each, with the switches a
handle reads at creation resolved as gpx_create resolves them.  Checked here: the defaults and the set of names against
INTEGRATION.md §7, the set of names against the string literals of gpx_env.h, every validity rule at its edges (set
through os.environ, so a change made from Python reaches the next snapshot), and that no other source of the library
calls getenv.
"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianprocesspathmodelling_amd", "csrc")


@pytest.fixture
def snapshot(gpx, monkeypatch):
    """snapshot(NAME=value, ...) -> {name: printed value} with exactly those GPX_* variables set"""
    for name in [n for n in os.environ if n.startswith("GPX_")]:
        monkeypatch.delenv(name)

    def take(**env):
        with monkeypatch.context() as m:
            for name, value in env.items():
                m.setenv(name, value)
            n = gpx.gpx_debug_env(None, 0)
            buf = C.create_string_buffer(n + 1)
            assert gpx.gpx_debug_env(buf, n + 1) == n
        lines = buf.value.decode().splitlines()
        assert all(re.fullmatch(r"GPX_[A-Z_]+=.*", ln) for ln in lines), lines
        names = [ln.split("=", 1)[0] for ln in lines]
        assert len(set(names)) == len(names)
        return dict(ln.split("=", 1) for ln in lines)

    return take


def documented_table():
    """{name: (default, read at)} of the table of INTEGRATION.md §7"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    text = text[text.index("## 7. Environment switches"):]
    rows = {}
    for line in text.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        m = re.fullmatch(r"`(GPX_[A-Z_]+)`", cells[0])
        if line.startswith("|") and m:
            assert m.group(1) not in rows
            rows[m.group(1)] = (cells[1].strip("`"), cells[2])
    return rows


def test_defaults_are_the_documented_ones(snapshot):
    doc, snap = documented_table(), snapshot()
    assert set(snap) == set(doc)
    assert snap == {name: dflt for name, (dflt, _) in doc.items()}
    assert {at for _, at in doc.values()} == {"create", "call", "process"}


def test_names_are_the_string_literals_of_the_one_header(snapshot):
    src = open(os.path.join(CSRC, "gpx_env.h")).read()
    assert set(snapshot()) == set(re.findall(r'"(GPX_[A-Z_]+)"', src))


def test_moments_in_the_table_are_those_of_the_header():
    src = open(os.path.join(CSRC, "gpx_env.h")).read()
    header = dict(re.findall(r'X\("(GPX_[A-Z_]+)", \w+, \w+, (create|call|process),', src))
    assert header == {name: at for name, (_, at) in documented_table().items()}


@pytest.mark.parametrize("name, cases", [
    ("GPX_DIAG_STEP", {"64": "64", "32": "128", "128": "128"}),
    ("GPX_CU_SELF_RESERVE", {"0": "0", "1": "1", "4": "4", "5": "0", "-1": "0"}),
    ("GPX_PRED_BATCH", {"127": "8192", "128": "128", "1000": "896", "4194304": "4194304", "4194305": "8192"}),
    # unset: the library follows the fit's panel width; set at all — valid or not — it never does ("was set")
    ("GPX_NB_PRED", {None: "unset", "100": "1024", "128": "128", "4096": "4096", "4224": "1024"}),
    ("GPX_NB_SHARD", {"64": "0", "128": "128", "2048": "2048", "2176": "0", "200": "0"}),
    ("GPX_NB_SOLVE", {"100": "256", "128": "128", "4096": "4096", "4224": "256"}),
    ("GPX_NB_GRAD", {"100": "0", "128": "128", "4096": "4096", "4224": "0"}),
    ("GPX_NB_WIDE_FROM", {"0": "0", "40960": "40960", "4096": "4096"}),
    ("GPX_REST_SPLIT", {"0": "0", "16": "16", "-3": "-3"}),
    ("GPX_RESV_CHAIN", {"0": "0", "2": "2"}),
    ("GPX_RESV_FORM", {"0": "0", "1": "1"}),
    ("GPX_CHAIN_FLAG", {None: "unset", "0": "0", "1": "1"}),
    ("GPX_SHARD_TWO_PIPE", {None: "unset", "0": "0", "1": "1"}),
    ("GPX_SHARD_REPLICATE", {None: "unset", "0": "0", "1": "1"}),
    ("GPX_SPLIT_STRIP", {None: "1", "": "0", "0": "0", "1": "1", "x": "0"}),   # on by default
    ("GPX_FUSED_STRIP", {None: "0", "": "0", "0": "0", "1": "1", "x": "0"}),   # off by default
    ("GPX_SHARD_DEAL", {None: "1", "cyclic": "0", "0": "0", "snake": "1", "1": "1"}),
    ("GPX_MICROBENCH_ITERS", {"63": "65536", "64": "64", "1048576": "1048576", "1048577": "65536"}),
    ("GPX_RCCL_PATH", {None: "unset", "/some/where/librccl.so": "/some/where/librccl.so"}),
])
def test_validity_rules_at_their_edges(snapshot, name, cases):
    defaults = snapshot()
    for value, want in cases.items():
        got = snapshot(**({} if value is None else {name: value}))
        assert got[name] == want, (name, value)
        assert {k: v for k, v in got.items() if k != name} == {k: v for k, v in defaults.items() if k != name}


def test_a_small_buffer_is_cut_and_terminated(gpx, snapshot):
    n = len("".join(f"{k}={v}\n" for k, v in snapshot().items()))
    buf = C.create_string_buffer(b"\xff" * 32, 32)
    assert gpx.gpx_debug_env(buf, 16) == n
    assert buf.raw[15:17] == b"\x00\xff" and buf.value == b"GPX_DIAG_STEP=1"
    assert gpx.gpx_debug_env(None, 100) == n and gpx.gpx_debug_env(buf, 0) == n


def test_only_the_one_header_reads_the_environment():
    hits = [f for f in sorted(os.listdir(CSRC))
            if f.endswith((".hip", ".h", ".inc", ".cpp")) and "getenv(" in open(os.path.join(CSRC, f)).read()]
    assert hits == ["gpx_env.h"]
