"""GPU: the device-flag hand-over between the library's streams tests itself.

The diagonal chain of the blocked Cholesky hands over to its side stream through a device word a parked kernel polls
(csrc/gpx_api.hip: diag_enqueue).  That needs kernels of different streams to run concurrently.  Where they do not —
AMD_SERIALIZE_KERNEL, one hardware queue, counter collection — round 3 spun for 15 s and failed the fit; now the
handle runs a ~100 us handshake at its first fit (flag_handover_probe: bounded at ~50 ms) and hands over by hipEvents
when the handshake does not complete.  Same kernels and arithmetic either way: the results must agree with the oracle
at north_star's 1e-6 AND be bit-identical between the two hand-overs.

The serialised runs live in child processes (the HIP runtime reads its environment once).
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from gaussianprocesspathmodelling_amd import GP
from oracle.gp_oracle import OracleGP, synthetic_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys, time
import numpy as np
sys.path.insert(0, {root!r})
from gaussianprocesspathmodelling_amd import GP
from oracle.gp_oracle import synthetic_problem
X, y, Xs = synthetic_problem(3000, 3, 300, seed=11)
t0 = time.time()
with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0, block=512) as gp:
    mean, var = gp.fit(X, y).predict(Xs)
    tm = dict(gp.timings_)
    m1, v1 = gp.fit_predict(X, y, Xs)
np.save({out!r}, np.stack([mean, var, m1, v1]))
print(json.dumps({{"seconds": time.time() - t0, "handover_flags": tm["handover_flags"],
                  "handover_retries": tm["handover_retries"], "info": gp.info_}}))
"""


def run_child(tmp_path, env_extra):
    out = str(tmp_path / "res.npy")
    env = dict(os.environ)
    env.pop("GPX_CHAIN_FLAG", None)
    env.update(env_extra)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, out=out)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    rec["wall"] = time.time() - t0
    return rec, np.load(out)


def reference():
    X, y, Xs = synthetic_problem(3000, 3, 300, seed=11)
    ref = OracleGP("rbf", 0.25, 1.5, 1e-2, jitter=0.0).fit(X, y)
    return ref.predict(Xs)


def check(res, mr, vr):
    for mean, var in ((res[0], res[1]), (res[2], res[3])):
        assert np.max(np.abs(mean - mr) / np.maximum(np.abs(mr), 1e-6)) <= 1e-6
        assert np.max(np.abs(var - vr) / np.maximum(vr, 1e-6 * 1.5)) <= 1e-6


def test_default_handle_uses_device_flags_and_forced_events_are_bit_identical(tmp_path):
    mr, vr = reference()
    rec, res = run_child(tmp_path, {})
    assert rec["info"] == 0 and rec["handover_flags"] == 1.0 and rec["handover_retries"] == 0.0
    check(res, mr, vr)
    rec0, res0 = run_child(tmp_path, {"GPX_CHAIN_FLAG": "0"})
    assert rec0["handover_flags"] == 0.0
    assert np.array_equal(res, res0)            # the hand-over changes no bit


@pytest.mark.parametrize("env", [{"AMD_SERIALIZE_KERNEL": "3"}, {"GPU_MAX_HW_QUEUES": "1"}])
def test_serialised_kernels_fall_back_to_events_without_a_stall(tmp_path, env):
    mr, vr = reference()
    rec, res = run_child(tmp_path, env)
    assert rec["info"] == 0
    check(res, mr, vr)
    # no 15 s time-out of a parked stream (round 3's failure mode), and no fit had to be re-run
    assert rec["seconds"] < 10.0, rec
    assert rec["handover_retries"] == 0.0
    if "AMD_SERIALIZE_KERNEL" in env:           # every launch waits for the previous one: the handshake cannot complete
        assert rec["handover_flags"] == 0.0
    # whatever the probe chose, the bits are those of the default run
    _, res_default = run_child(tmp_path, {})
    assert np.array_equal(res, res_default)


def test_in_process_default_reports_its_handover():
    X, y, Xs = synthetic_problem(2000, 3, 100, seed=4)
    with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0) as gp:
        gp.fit(X, y)
        flags = gp.timings_["handover_flags"]
        assert flags == (0.0 if os.environ.get("GPX_CHAIN_FLAG") == "0" or os.environ.get("ROCPROF_COUNTER_COLLECTION") else 1.0)


def test_chain_flag_switched_between_fits_of_one_handle(monkeypatch):
    """GPX_CHAIN_FLAG is read at the start of every call: the same handle hands over by hipEvents in the fit after it was
    set to 0 and by device flags again after 1, and the three factorisations (six 256-wide panels) agree bit for bit."""
    monkeypatch.delenv("GPX_CHAIN_FLAG", raising=False)
    X, y, _ = synthetic_problem(1536, 2, 8, seed=5)
    with GP("rbf", 0.25, 1.5, 1e-2, jitter=0.0, block=256) as gp:
        gp.fit(X, y)
        first = (gp.alpha_.copy(), gp.log_det_)
        for value in ("0", "1"):
            monkeypatch.setenv("GPX_CHAIN_FLAG", value)
            gp.fit(X, y)
            assert gp.timings_["handover_flags"] == float(value)
            assert np.array_equal(gp.alpha_, first[0]) and gp.log_det_ == first[1]
