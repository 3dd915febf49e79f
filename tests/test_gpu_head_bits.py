"""The classifier heads give the bits they gave before their kernels were unified.

``tests/golden/head_bits.json`` maps a case name to the SHA-256 of the raw bytes of what the public wrappers
(``ddpx.ops.head.head_forward`` / ``head_backward`` and ``ddpx.ops.f32.head_forward`` / ``head_backward``) return
for that case.  It was recorded once, with this module run as a script, on a build of the commit before the two
bf16 forward kernels, the two backward entry points and the fp32 head's kernel copies became one each; it is never
regenerated from the code under test.  A digest that differs means a summation order or an FMA contraction changed.

Inputs: ``torch.randn`` from a seeded CPU generator, cast to the operand dtype (the weights scaled by K^-1/2 so the
softmax is not saturated and every bit of dlogits counts), labels from ``torch.randint``, ``lam`` in (0, 1).
The shapes: by ``head_ksplit`` (M, K) = (1, 32), (17, 160), (50, 512), (17, 1024), (17, 2048) run 1, 1, 4, 8 and
16 K slices (no hand-off, one and two rounds of the 8-wide partial sum, a ragged last row block); the fp32 backward
at M = 1000, NC = 10 is past the LDS stage of dlogits, and K = 100 leaves a partial 64-column block.
"""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_bits.json")


def _digest(*tensors):
    sha = hashlib.sha256()
    for t in tensors:
        sha.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return sha.hexdigest()


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _fwd_inputs(dev, C, M, K, dtype, tag):
    g = _gen(tag, C, M, K)
    h = torch.randn(M, K, generator=g).to(dtype).to(dev)
    w = (torch.randn(C, K, generator=g) * K ** -0.5).to(dtype).to(dev)
    b = (torch.randn(C, generator=g) * 0.1).to(dev)
    a = torch.randint(0, C, (M,), generator=g).to(dev)
    tb = torch.randint(0, C, (M,), generator=g).to(dev)
    lam = (torch.rand(M, generator=g) * 0.98 + 0.01).to(dev)
    return h, w, b, a, tb, lam


def _soft(tb, lam, soft):
    from ddpx.ops.loss import SoftTargets
    return {"soft": SoftTargets(tb, lam, 0.1)} if soft else {}


# ------------------------------------------------------------------ bf16 forward
def bf16_fwd(dev, C, M, K, soft):
    from ddpx.ops.head import head_forward
    h, w, b, a, tb, lam = _fwd_inputs(dev, C, M, K, torch.bfloat16, 1)
    hits = torch.zeros((), dtype=torch.int32, device=dev)
    loss, logits, dl = head_forward(h, w, b, a, correct=hits, **_soft(tb, lam, soft))
    return _digest(loss, logits, dl, hits)


def bf16_fwd_lr(dev):
    """The LR-table advance in the forward launch, through both row finishes (C = 10 and C = 100)."""
    from ddpx.ops.head import head_forward
    out = []
    for C in (10, 100):
        h, w, b, a, _, _ = _fwd_inputs(dev, C, 50, 512, torch.bfloat16, 2)
        table = torch.tensor([0.5, 0.25, 0.125], device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        lr = torch.zeros(1, device=dev)
        for _ in range(2):
            loss, _, _ = head_forward(h, w, b, a, want_logits=False, lr_advance=(table, counter, lr))
            out += [loss, lr.clone(), counter.clone()]
    return _digest(*out)


# ------------------------------------------------------------------ bf16 backward
def bf16_bwd(dev, mode, C, M, K):
    from ddpx.ops.head import head_backward
    g = _gen(3, C, M, K)
    dl = (torch.randn(M, C, generator=g) / M).to(dev)
    h = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(C, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
    old = [torch.randn(s, generator=g) * 0.1 for s in ((C, K), (C,), (K,))]
    mom = [torch.randn(s, generator=g) * 0.01 for s in ((C, K), (C,), (K,))]
    go = torch.tensor(0.5, device=dev)
    dH = torch.empty(M, K, dtype=torch.bfloat16, device=dev)
    if mode == "sgd":  # fused SGD with momentum; the bf16 copy of W is the W operand itself, as in training
        lr = torch.tensor(0.1, device=dev)
        ms = [o.to(dev) for o in old]
        ms[0] = w.float()
        bs = [m.to(dev) for m in mom]
        sh = [m.to(torch.bfloat16) for m in ms]
        sgd = [(p, m, s, lr, 0.9, 5e-4) for p, m, s in zip(ms, bs, sh)]
        head_backward(dl, go, h, sh[0], None, None, dH=dH, relu_mask=True, dh_scale=2.0, sgd_w=sgd[0], sgd_b=sgd[1],
                      sgd_prev=sgd[2])
        return _digest(dH, *ms, *bs, *sh)
    gdt, acc = (torch.float32, False) if mode == "f32" else (torch.bfloat16, True)
    dW, db, dbp = (o.to(gdt).to(dev) for o in old)
    head_backward(dl, go, h, w, dW, db, dH=dH, dbprev=dbp, relu_mask=True, accumulate=acc, dh_scale=2.0)
    return _digest(dW, db, dH, dbp)


# ------------------------------------------------------------------ fp32
def f32_fwd(dev, NC, M, K, soft):
    from ddpx.ops import f32
    h, w, b, a, tb, lam = _fwd_inputs(dev, NC, M, K, torch.float32, 4)
    loss, logits, dl = f32.head_forward(h, w, b, a, **_soft(tb, lam, soft))
    return _digest(loss, logits, dl)


def f32_bwd(dev, NC, M, K):
    from ddpx.ops import f32
    g = _gen(5, NC, M, K)
    dl = (torch.randn(M, NC, generator=g) / M).to(dev)
    h = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(NC, K, generator=g) * K ** -0.5).to(dev)
    dW, db = torch.empty(NC, K, device=dev), torch.empty(NC, device=dev)
    dh = f32.head_backward(dl, torch.tensor(0.5, device=dev), h, w, dW, db, relu_mask=True, dh_scale=2.0)
    return _digest(dW, db, dh)


def _cases():
    out = {}
    for C in (1, 10, 12, 16, 17, 100, 128):
        for M, K in ((1, 32), (17, 160), (50, 512), (17, 1024), (17, 2048)):
            for soft in (False, True):
                out[f"bf16_fwd_{'soft' if soft else 'hard'}_C{C}_M{M}_K{K}"] = (bf16_fwd, C, M, K, soft)
    out["bf16_fwd_lr_advance"] = (bf16_fwd_lr,)
    for mode in ("f32", "bf16acc", "sgd"):
        for C in (10, 12, 100):
            for M in (7, 300):
                for K in (32, 160):
                    out[f"bf16_bwd_{mode}_C{C}_M{M}_K{K}"] = (bf16_bwd, mode, C, M, K)
    for NC in (10, 12, 16, 17, 100):
        for M, K in ((1, 32), (50, 160)):
            for soft in (False, True):
                out[f"f32_fwd_{'soft' if soft else 'hard'}_NC{NC}_M{M}_K{K}"] = (f32_fwd, NC, M, K, soft)
    for NC in (10, 12, 100):
        for M in (7, 300, 1000):
            for K in (64, 100):
                out[f"f32_bwd_NC{NC}_M{M}_K{K}"] = (f32_bwd, NC, M, K)
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_bits(gpu, golden, name):
    fn, *args = CASES[name]
    assert fn(gpu, *args) == golden[name], name


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dev = torch.device("cuda", 0)
    rec = {name: fn(dev, *args) for name, (fn, *args) in CASES.items()}
    dst = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} digests to {dst}")
