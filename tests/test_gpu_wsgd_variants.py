"""The non-default variants of the warp-specialised weight-gradient + SGD kernel (csrc/include/ddpx_wgrad_sgd.h).

The variables that select a variant are read once per process, so each case runs in a fresh child process with its
variables set: one single launch (320 tiles of 64x128 on 256 CUs: some workgroups own two tiles and some one, so the
ring crosses a tile boundary and both the hand-off and the drain run) and one pair launch (160 + 120 tiles: workgroups
straddle both GEMMs), each compared bit for bit with the fp32 weight gradient from the GEMM + the flat SGD pass.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import sys

import torch

from ddpx.ops import gemm as G
from ddpx.ops.elementwise import sgd_flat_

mode = sys.argv[1]  # equal | math (probe 3: nothing is updated) | stream (probe 4: zero gradients)
dev = torch.device("cuda", 0)
K, MOM, WD = 512, 0.9, 5e-4
torch.manual_seed(21)
lr = torch.full((), 0.05, device=dev)


def make(M, N):
    """Operands and initial state of dW[M, N] = dy^T x, and the expected (master, momentum, shadow)."""
    dy = torch.randn(K, M, device=dev).to(torch.bfloat16)
    x = torch.randn(K, N, device=dev).to(torch.bfloat16)
    p = torch.randn(M * N, device=dev) * 0.02
    b = torch.randn(M * N, device=dev) * 0.01
    sent = torch.full((M * N,), 123.0, dtype=torch.bfloat16, device=dev)
    # the reference first (default kernels), so the child's first launch is never a probe
    g = torch.empty(M, N, device=dev)
    G.linear_wgrad(dy, x, g)
    if mode == "stream":
        g.zero_()
    pr, br, sr = p.clone(), b.clone(), torch.empty_like(sent)
    sgd_flat_(pr, br, g.view(-1), sr, lr, MOM, WD)
    expect = (p.clone(), b.clone(), sent.clone()) if mode == "math" else (pr, br, sr)
    return dy, x, (p, b, sent), expect


def check(what, state, expect):
    torch.cuda.synchronize()
    for name, a, e in zip(("master", "momentum", "shadow"), state, expect):
        assert torch.equal(a, e), (what, name)


dy, x, st, expect = make(1024, 2560)
G.linear_wgrad(dy, x, None, sgd=(st[0], st[1], st[2], lr, MOM, WD))
check("single", st, expect)

dy0, x0, st0, expect0 = make(512, 2560)
dy1, x1, st1, expect1 = make(768, 1280)
assert G.wgrad_sgd_pair(dy0, x0, (st0[0], st0[1], st0[2], lr, MOM, WD),
                        dy1, x1, (st1[0], st1[1], st1[2], lr, MOM, WD)) is True
check("pair 0", st0, expect0)
check("pair 1", st1, expect1)
print("variant ok")
'''

_VARIANTS = [
    ({"DDPX_WSGD_ORDER": "m"}, "equal"),
    ({"DDPX_WSGD_MATH_WAVES": "4"}, "equal"),
    ({"DDPX_WSGD_STREAM_WAVES": "8"}, "equal"),
    ({"DDPX_WSGD_STAGES": "4"}, "equal"),
    ({"DDPX_WSGD_STAGES": "4", "DDPX_WSGD_STREAM_WAVES": "8"}, "equal"),  # the wide-MLP production kernel
    ({"DDPX_WSGD_XTRA": "3"}, "math"),
    ({"DDPX_WSGD_XTRA": "4"}, "stream"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("env,mode", _VARIANTS, ids=[",".join(f"{k[10:]}={v}" for k, v in e.items())
                                                     for e, _ in _VARIANTS])
def test_wsgd_variant_matches_unfused(gpu, env, mode):
    """Single and pair launches of one variant == fp32 dW from the GEMM + the flat SGD pass, bit for bit (master,
    momentum, bf16 shadow).  The math-only probe must leave all three untouched (shadow pre-filled with a sentinel);
    the stream-only probe must equal the flat SGD pass on an all-zero gradient."""
    base = {k: v for k, v in os.environ.items() if not k.startswith("DDPX_WSGD_")}
    r = subprocess.run([sys.executable, "-c", _CHILD, mode], cwd=ROOT, env=dict(base, PYTHONPATH=ROOT, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "variant ok" in r.stdout, r.stdout[-4000:]
