"""The plan query of the warp-specialised weight-gradient + SGD kernel (``ddpx_wgrad_sgd_plan``, host-only code):
which tile height, ring depth and wave counts a launch would run, by default and under each ``DDPX_WSGD_*`` knob.

The knobs are read once per process, so every environment runs in a fresh child process.  256 CUs are assumed when
no GPU is present (as the launch code does).  Skipped when the native library has not been built.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = os.path.join(ROOT, "ddpx", "_native", "libddpx_kernels.so")

pytestmark = pytest.mark.skipif(not os.path.exists(_LIB), reason="native library not built")

_CHILD = r'''
import json

from ddpx.ops import gemm as G

H, D0, W = 4096, 3072, 16384
print("PLANS " + json.dumps({
    "toy": G.wgrad_sgd_plan(H, H, H, D0),            # fc1 + fc0 of the 3072-4096-4096-10 MLP, batch 512
    "wide": G.wgrad_sgd_plan(W, W, W, D0),           # the wide MLP's pair: 76 128-row tiles per CU
    "toy_fp8": G.wgrad_sgd_plan(H, H, H, D0, fp8=True),
    "toy_fp8_t": G.wgrad_sgd_plan(H, H, H, D0, fp8=True, transposed=True),
    "odd_m": G.wgrad_sgd_plan(H + 64, H, H, D0),     # M % 128 == 64 in one GEMM of the pair
    "few_tiles": G.wgrad_sgd_plan(1024, 2560),       # 160 128-row tiles: fewer than CUs
    "single_fc1": G.wgrad_sgd_plan(H, H),
    "bad_k": G.wgrad_sgd_plan(H, H, H, D0, K=256),
    "bad_m": G.wgrad_sgd_plan(100, 256),
}))
'''


def _plans(env):
    base = {k: v for k, v in os.environ.items() if not k.startswith("DDPX_WSGD_")}
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=dict(base, PYTHONPATH=ROOT, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PLANS ")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0][6:])


def _v(bm, stages, nsw, nmw):
    return {"bm": bm, "stages": stages, "nsw": nsw, "nmw": nmw}


def test_plan_defaults():
    p = _plans({})
    assert p["toy"] == _v(128, 3, 4, 8)        # the 128-row tile is the toy pair's default
    assert p["single_fc1"] == _v(128, 3, 4, 8)
    assert p["wide"] == _v(128, 3, 4, 8)       # ... and the wide pair's
    assert p["toy_fp8"] == _v(64, 3, 4, 8)     # MX-FP8 copies: 64 rows
    assert p["toy_fp8_t"] == _v(64, 3, 8, 4)   # the transposed copy needs the 8-stream-wave layout
    assert p["odd_m"] == _v(64, 3, 4, 8)
    assert p["few_tiles"] == _v(64, 3, 4, 8)   # not every CU would get a 128-row tile
    assert p["bad_k"] is None and p["bad_m"] is None


@pytest.mark.parametrize("env,toy,wide,few", [
    ({"DDPX_WSGD_TILE": "64"}, _v(64, 3, 4, 8), _v(64, 4, 8, 4), _v(64, 3, 4, 8)),
    # forced 128: also where the default would not pick it ...
    ({"DDPX_WSGD_TILE": "128"}, _v(128, 3, 4, 8), _v(128, 3, 4, 8), _v(128, 3, 4, 8)),
    # the 128-row tile exists in one layout only: any knob that leaves it selects a 64-row kernel
    ({"DDPX_WSGD_STAGES": "4"}, _v(64, 4, 4, 8), _v(64, 4, 8, 4), _v(64, 4, 4, 8)),
    ({"DDPX_WSGD_STREAM_WAVES": "8"}, _v(64, 3, 8, 4), _v(64, 4, 8, 4), _v(64, 3, 8, 4)),
    ({"DDPX_WSGD_MATH_WAVES": "4"}, _v(64, 3, 4, 4), _v(64, 4, 8, 4), _v(64, 3, 4, 4)),
    ({"DDPX_WSGD_ORDER": "m"}, _v(64, 3, 4, 4), _v(64, 4, 8, 4), _v(64, 3, 4, 4)),
], ids=["TILE=64", "TILE=128", "STAGES=4", "STREAM_WAVES=8", "MATH_WAVES=4", "ORDER=m"])
def test_plan_knobs(env, toy, wide, few):
    p = _plans(env)
    assert p["toy"] == toy
    assert p["wide"] == wide
    assert p["few_tiles"] == few
    # ... but never for MX-FP8 copies or M % 128 == 64, whatever the knob says
    assert p["toy_fp8"]["bm"] == 64 and p["toy_fp8_t"]["bm"] == 64 and p["odd_m"]["bm"] == 64
