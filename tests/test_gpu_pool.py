"""The device-memory pool against the real driver, once: tests/test_pool_cpu.py holds the allocator to its rules on a CPU; here
the solves of tests/test_gpu_amg.py::test_results_do_not_depend_on_what_recycled_device_memory_holds run in two child processes,
with the default knobs and with a pool of 0.05 GB and arenas of 192 MiB, and report the pool's own counters
(femshell_pool_stats) after every solve and after the last context is closed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu

SCRIPT = r'''
import importlib, json, os, sys
import numpy as np
sys.path.insert(0, %r)
from tests.helpers import meshes
pkg = importlib.import_module("fem-shell_amd")
out, stats = {}, []
for kind in ("panel", "quads"):
    m = meshes.structured(40, 40, 0, 0, 10, 10, kind="t" if kind == "panel" else "q", ul_lr=True, bcids=(0, 0, 0, 0) if kind == "panel" else (1, 1, 1, 1), factor=300.0, loading=2)
    fs = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    u, info = fs.solve(rtol=1e-10, max_it=20000)
    out[kind + "_jacobi"] = u
    stats.append([kind + "_jacobi", pkg.pool_stats()])
    for where in ("device", "host"):
        os.environ["FEMSHELL_AMG_SYMBOLIC"] = where
        dm = m.dirichlet_mask()
        dm[m.n_nodes // 2 + (1 if where == "host" else 0)] = 0x3F   # K changes: the hierarchy is rebuilt
        fs.set_dirichlet(dm)
        fs.set_preconditioner("amg", coarsest_nodes=60)
        u, info = fs.solve(rtol=1e-10, max_it=500)
        assert info["converged"] == 1
        out[kind + "_amg_" + where] = u
        out[kind + "_hist_" + where] = fs.residual_history()
        stats.append([kind + "_amg_" + where, pkg.pool_stats()])
    fs.close()
    stats.append([kind + "_closed", pkg.pool_stats()])
np.savez(sys.argv[1], **out)
with open(sys.argv[2], "w") as f:
    json.dump(stats, f)
''' % (ROOT,)

KNOBS = {"default": {}, "tight": {"FEMSHELL_POOL_GB": "0.05", "FEMSHELL_POOL_ARENA_MB": "192"}}
LIMIT = {"default": 24 << 30, "tight": int(0.05 * 1073741824.0)}
ARENA = {"default": 512 << 20, "tight": 192 << 20}


def test_pool_counters_on_the_device_and_results_whatever_the_pool_keeps(tmp_path):
    """The same bits from both runs (the pool must not change results).  After each solve, with the context alive and no setup
    in progress, rule 5 as far as the six counters show it: nothing waits, what is kept is within FEMSHELL_POOL_GB, the arenas are
    whole arenas the size asked for or kept blocks that were carved, and the driver holds exactly the kept blocks, the arenas and
    the directly allocated buffers in use -- between kept + arenas and kept + arenas + in use.  After close() of the last context
    every counter is zero."""
    ensure_built()
    results, stats = {}, {}
    for name, knobs in KNOBS.items():
        npz, js = str(tmp_path / (name + ".npz")), str(tmp_path / (name + ".json"))
        env = {k: v for k, v in os.environ.items() if not k.startswith("FEMSHELL_POOL_")}
        env.update(knobs, FEMSHELL_AMG_DEVICE_MIN="100")
        r = subprocess.run([sys.executable, "-c", SCRIPT, npz, js], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        results[name] = np.load(npz)
        with open(js) as f:
            stats[name] = json.load(f)
    a, b = results["default"], results["tight"]
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 10
    for k in a.files:
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for name in KNOBS:
        assert [s[0] for s in stats[name]] == [kind + step for kind in ("panel", "quads") for step in ("_jacobi", "_amg_device", "_amg_host", "_closed")]
        for step, c in stats[name]:
            print(name, step, c)
            if step.endswith("_closed"):
                assert all(v == 0 for v in c.values()), (name, step, c)
                continue
            assert c["pending"] == 0 and c["live"] > 0, (name, step, c)
            assert c["cached"] <= LIMIT[name], (name, step, c)
            assert c["cached"] + c["arena_bytes"] <= c["outstanding"] <= c["cached"] + c["arena_bytes"] + c["live"], (name, step, c)
            assert c["arenas"] >= 1 and c["arena_bytes"] >= ARENA[name], (name, step, c)
