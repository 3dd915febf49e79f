"""The 128-row tile of the warp-specialised weight-gradient + SGD kernel (csrc/include/ddpx_wgrad_sgd.h): 128x128 math
tiles handed to the optimizer stream through ONE LDS buffer.

``DDPX_WSGD_TILE`` is read once per process, so the launches run in child processes: one with ``DDPX_WSGD_TILE=128``
and one with ``=64`` run every shape case on the same seeded inputs (shared by all tests of this module), two more run
the math-only / stream-only probes.  A child compares master, momentum and bf16 shadow of every case with
``torch.equal`` against the fp32 weight gradient from ``G.linear_wgrad`` + ``sgd_flat_``, reports the tile height the
plan query gives for the case, and prints the SHA-256 of each array's bytes; the test compares the two children's
digests (equal digests = equal bytes: the bitwise comparison across the two processes).

Shapes (K = 512; tile counts are 128x128 tiles, 256 CUs):
  one_tile       128x128                      grid of 1: fill and drain are the whole launch
  single_320     2048x2560                    1 and 2 tiles per workgroup: the ring crosses a tile boundary
  pair_straddle  1024x2560 + 1536x1280        160 + 120 tiles: workgroups whose tile list spans both GEMMs
  pair_mom0      the same pair, momentum 0    the momentum stream aliases the master
  pair_640       2048x2560 + 2048x2560        3 tiles in some workgroups: the single buffer reused twice or more
  not_eligible   192x256 (M % 128 == 64)      must run the 64-row kernel under DDPX_WSGD_TILE=128 too
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import hashlib
import json
import sys

import torch

from ddpx.ops import gemm as G
from ddpx.ops.elementwise import sgd_flat_

mode = sys.argv[1]  # equal | math (probe 3: nothing is updated) | stream (probe 4: zero gradients)
names = sys.argv[2].split(",")
dev = torch.device("cuda", 0)
K, WD = 512, 5e-4
lr = torch.full((), 0.05, device=dev)
CASES = {
    "one_tile": ([(128, 128)], 0.9),
    "single_320": ([(2048, 2560)], 0.9),
    "pair_straddle": ([(1024, 2560), (1536, 1280)], 0.9),
    "pair_mom0": ([(1024, 2560), (1536, 1280)], 0.0),
    "pair_640": ([(2048, 2560), (2048, 2560)], 0.9),
    "not_eligible": ([(192, 256)], 0.9),
}


def make(M, N, mom):
    """Operands and initial state of dW[M, N] = dy^T x, and the expected (master, momentum, shadow)."""
    dy = torch.randn(K, M, device=dev).to(torch.bfloat16)
    x = torch.randn(K, N, device=dev).to(torch.bfloat16)
    p = torch.randn(M * N, device=dev) * 0.02
    b = torch.randn(M * N, device=dev) * 0.01
    sent = torch.full((M * N,), 123.0, dtype=torch.bfloat16, device=dev)
    g = torch.empty(M, N, device=dev)
    G.linear_wgrad(dy, x, g)  # stored fp32 gradient: the tile GEMM, no fused optimizer
    if mode == "stream":
        g.zero_()
    pr, br, sr = p.clone(), b.clone(), torch.empty_like(sent)
    sgd_flat_(pr, br if mom else pr, g.view(-1), sr, lr, mom, WD)
    expect = (p.clone(), b.clone(), sent.clone()) if mode == "math" else (pr, br, sr)
    return dy, x, (p, b, sent), expect


def digest(t):
    return hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


for name in names:
    shapes, mom = CASES[name]
    torch.manual_seed(128)
    ops = [make(M, N, mom) for M, N in shapes]
    sg = [(st[0], st[1] if mom else None, st[2], lr, mom, WD) for _, _, st, _ in ops]
    if len(ops) == 1:
        (M0, N0), (M1, N1) = shapes[0], (0, 0)
        G.linear_wgrad(ops[0][0], ops[0][1], None, sgd=sg[0])
        launched = True
    else:
        (M0, N0), (M1, N1) = shapes
        launched = G.wgrad_sgd_pair(ops[0][0], ops[0][1], sg[0], ops[1][0], ops[1][1], sg[1]) is True
    torch.cuda.synchronize()
    plan = G.wgrad_sgd_plan(M0, N0, M1, N1, K)
    bad = [f"gemm {i} {what}" for i, (_, _, st, ex) in enumerate(ops)
           for what, a, e in zip(("master", "momentum", "shadow"), st, ex) if not torch.equal(a, e)]
    print("CASE " + json.dumps({"case": name, "launched": launched, "plan": plan, "mismatch": bad,
                                "digest": [digest(a) for _, _, st, _ in ops for a in st]}), flush=True)
print("children ok")
'''

_EQUAL_CASES = ["one_tile", "single_320", "pair_straddle", "pair_mom0", "pair_640", "not_eligible"]


def _run_child(env, mode, cases):
    base = {k: v for k, v in os.environ.items() if not k.startswith("DDPX_WSGD_")}
    r = subprocess.run([sys.executable, "-c", _CHILD, mode, ",".join(cases)], cwd=ROOT,
                       env=dict(base, PYTHONPATH=ROOT, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=180)
    assert r.returncode == 0 and "children ok" in r.stdout, r.stdout[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            d = json.loads(line[5:])
            out[d["case"]] = d
    assert sorted(out) == sorted(cases), r.stdout[-4000:]
    return out


@pytest.fixture(scope="module")
def runs(gpu):
    """Every shape case once per tile height: {128: {case: report}, 64: {case: report}}."""
    return {t: _run_child({"DDPX_WSGD_TILE": str(t)}, "equal", _EQUAL_CASES) for t in (128, 64)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", _EQUAL_CASES)
def test_tile128_matches_unfused_and_tile64(runs, case):
    """The 128-row kernel == fp32 dW from the GEMM + the flat SGD pass == the 64-row kernel, bit for bit (master,
    momentum, bf16 shadow), and the plan query proves which kernel each child ran: a silent fall-back to the 64-row
    kernel fails here.  M % 128 == 64 must take the 64-row kernel even when 128 is forced."""
    hi, lo = runs[128][case], runs[64][case]
    assert hi["launched"] and lo["launched"]
    assert hi["plan"] is not None and hi["plan"]["bm"] == (64 if case == "not_eligible" else 128), hi["plan"]
    assert lo["plan"] is not None and lo["plan"]["bm"] == 64, lo["plan"]
    assert hi["mismatch"] == [], hi["mismatch"]
    assert lo["mismatch"] == [], lo["mismatch"]
    assert hi["digest"] == lo["digest"]


@pytest.mark.gpu
@pytest.mark.parametrize("xtra,mode", [("3", "math"), ("4", "stream")])
def test_tile128_probes(gpu, xtra, mode):
    """The 128-row kernel's two measurement probes: math only leaves master, momentum and the (sentinel-filled)
    shadow untouched; stream only equals the flat SGD pass on an all-zero gradient."""
    out = _run_child({"DDPX_WSGD_TILE": "128", "DDPX_WSGD_XTRA": xtra}, mode, ["single_320"])["single_320"]
    assert out["plan"] is not None and out["plan"]["bm"] == 128, out["plan"]
    assert out["mismatch"] == [], out["mismatch"]
