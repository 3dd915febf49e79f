"""The model graphs of the fp32 recipe (``--dtype fp32``): VGG / ResNet-9, DeepNN and the MLP as sequences of the
operator wrappers of ``ops/f32.py``, each under the autograd node pair of ``ops/graph_node.py``.  The model walks
and the plan state shared with the bf16 graphs (``vgg_native.py``, ``deepnn_native.py``, ``mlp.py``) are in
``ops/plan.py``.

The fp32 masters in the flat parameter store are read directly (no compute shadow); gradients land in
``main_grad`` (DDP bucket storage) through the ``FlatParams`` grad protocol, so DDP, the flat SGD and
the checkpoint format are the same as on the bf16 path.

The operators are called through the module (``F.bn_backward``), so a debugging tool that wraps one in ``ops/f32.py``
sees the graphs' calls.
"""
from __future__ import annotations

import torch

from . import f32 as F
from ..models.resnet import tail_of
from .graph_node import Graph, LogitsNode, LossNode
from .plan import DeepNNPlanBase, _sync_comm, conv_blocks, plan_of


def _grad_write(flat, p, fn):
    """Run fn(out, accumulate) into p's gradient slot (DDP bucket storage) and announce it."""
    g, acc = flat.grad_target(p)
    fn(g, acc)
    flat.grad_done(p)


def prep_vgg_input(x):
    """NHWC fp32 with 4 channels (the loader's ``nhwc4_f32`` layout), or NCHW fp32 from a reference loader."""
    if x.dim() == 4 and x.shape[-1] == 4 and x.dtype == torch.float32:
        return x.contiguous()
    if x.dim() == 4 and x.shape[1] == 3:
        x = x.float().permute(0, 2, 3, 1)
        return torch.nn.functional.pad(x, (0, 1)).contiguous()
    raise ValueError(f"unsupported VGG input {tuple(x.shape)} {x.dtype}")


# ---------------------------------------------------------------------------------------------- prepared weights
class _ConvWeights:
    """The prepared fp32 weights of a network's 3x3 convolutions, per layer: ``uf`` / ``ud``, the Winograd F(2,3)
    transforms for the forward and the data gradient where Winograd applies at the planned input size (CIFAR's 32,
    halved by every pool), and ``wf`` / ``wd``, the layouts of the direct implicit GEMM.

    ``lazy_direct`` is the one rule the two networks do not share, and it changes which ``*_wprep`` launches run:

    * True (VGG / ResNet-9): a layer gets the direct layouts only where the plan needs them (no Winograd forward, or
      no Winograd data gradient).  A Winograd forward refreshes them exactly when they exist.  A forward at a size
      where Winograd does not apply allocates them on demand and gives up the layer's Winograd data gradient for
      good.
    * False (DeepNN): ``wf`` always exists (``wd`` wherever the direct data gradient takes the channel count), and a
      Winograd forward refreshes them when the layer has no Winograd data gradient.  The plan is never changed, so
      one forward at another input size (an eval) does not demote later 32x32 steps to the direct data gradient.
    """

    def __init__(self, convs_pools, dev, lazy_direct):
        self.lazy_direct = lazy_direct
        self.wf, self.wd, self.uf, self.ud = [], [], [], []

        def buf(n, wanted):
            return torch.empty(n, dtype=torch.float32, device=dev) if wanted else None
        H = 32
        for bi, (conv, pool) in enumerate(convs_pools):
            Co, Ci = conv.weight.shape[:2]
            Cp = F.conv_channels(Ci)
            wino = dev.type == "cuda" and F.wino_applies(H, H, Cp, Co)
            dwino = wino and bi > 0 and F.wino_applies(H, H, Co, Ci)  # the data gradient: Co -> Ci channels
            direct = not lazy_direct or not wino or (bi > 0 and not dwino)
            self.uf.append(buf(16 * Cp * Co, wino))
            self.ud.append(buf(16 * Co * Ci, dwino))
            self.wf.append(buf(9 * Cp * Co, direct))
            self.wd.append(buf(9 * Co * Ci, direct and Ci % 4 == 0))
            if pool:
                H //= 2

    def prep(self, bi, conv, x):
        """Refresh layer ``bi``'s prepared weights from ``conv.weight`` for a forward on ``x``.  True: the forward is
        Winograd's (``uf[bi]``); False: the direct GEMM's (``wf[bi]``).  The data gradient follows this forward's
        choice (:meth:`dgrad`)."""
        N, H, W, C = x.shape
        Co, Ci = conv.weight.shape[:2]
        wino = self.uf[bi] is not None and H == W and F.wino_applies(H, W, C, Co)
        if wino:
            F.wino_wprep(conv.weight, self.uf[bi], self.ud[bi])
            direct_dgrad = (self.wd[bi] is not None) if self.lazy_direct else (bi > 0 and self.ud[bi] is None)
            if direct_dgrad:
                F.conv_wprep(conv.weight, self.wf[bi], self.wd[bi])
            return True
        if self.wf[bi] is None:  # planned for Winograd at another input size: direct layouts on demand
            self.wf[bi] = torch.empty(9 * C * Co, dtype=torch.float32, device=x.device)
            self.wd[bi] = torch.empty(9 * Co * Ci, dtype=torch.float32, device=x.device)
            self.ud[bi] = None
        F.conv_wprep(conv.weight, self.wf[bi], self.wd[bi])
        return False

    def wino_dgrad(self, bi, wino):
        """Whether layer ``bi``'s data gradient is Winograd's, after a forward for which :meth:`prep` said ``wino``:
        ``ud[bi]`` was then made by that forward."""
        return wino and self.ud[bi] is not None

    def dgrad(self, bi, dy, N, H, W, C, Co, wino, mask=None):
        """The gradient [N,H,W,C] of layer ``bi``'s input.  ``mask`` (Winograd only): the ReLU output of the block
        below, applied in the epilogue."""
        if self.wino_dgrad(bi, wino):
            return F.wino_conv(dy.view(N, H, W, Co), self.ud[bi], C, mask=mask).view(N, H, W, C)
        return F.conv_dgrad(dy, self.wd[bi], N, H, W, C, Co)


# ---------------------------------------------------------------------------------------------- VGG, ResNet-9
class _VGGPlan(_ConvWeights):
    def __init__(self, model):
        self.blocks, self.skip = conv_blocks(model)
        self.skipped = {k for k in self.skip if k is not None}  # blocks whose output also feeds a skip connection
        super().__init__([(conv, pool) for conv, _, pool in self.blocks], model.classifier.weight.device,
                         lazy_direct=True)


def _vgg_plan(model):
    return plan_of(model, "_ddpx_plan_f32", _VGGPlan)


def _block_forward(plan, bi, x, training, comm, res=None):
    """One conv -> BatchNorm -> ReLU [-> pool] block: (output, what its backward needs).  ``res``: the skip operand
    added in the BatchNorm apply pass (the last block of a residual branch)."""
    conv, bn, pool = plan.blocks[bi]
    N, H, W, C = x.shape
    Co = conv.weight.shape[0]
    wino = plan.prep(bi, conv, x)
    if wino:
        y, st = F.wino_conv(x, plan.uf[bi], Co, stats=True) if training else (F.wino_conv(x, plan.uf[bi], Co), None)
    else:
        y, st = F.conv_fwd_stats(x, plan.wf[bi], Co) if training else (F.conv_fwd(x, plan.wf[bi], Co), None)
    xn, a, b, mean, rstd = F.bn_forward(y, N, H, W, Co, bn, training, pool, stats=st, comm=comm, res=res)
    return xn, (x, y, a, b, mean, rstd, (N, H, W, C, Co), wino)


def _vgg_forward(model, x, targets, training, soft=None):
    """VGG, and ResNet-9 through ``plan.skip``: the last block of a residual branch adds the skip operand in its
    BatchNorm apply pass."""
    plan = _vgg_plan(model)
    saved, outs = [], {}
    comm = _sync_comm(model, training)
    for bi in range(len(plan.blocks)):
        k = plan.skip[bi]
        x, sv = _block_forward(plan, bi, x, training, comm, res=None if k is None else outs.pop(k))
        saved.append(sv)
        if bi in plan.skipped:
            outs[bi] = x
    tail, scale = tail_of(model)
    feat = F.gmaxpool(x, scale) if tail == "max" else F.avgpool(x)
    cls = model.classifier
    loss, logits, dl = F.head_forward(feat, cls.weight, cls.bias, targets, soft)
    # the max tail's backward recomputes the argmax from the last block's output
    return saved, (x if tail == "max" else x.shape, feat), loss, logits, dl


def _vgg_backward(model, saved, last, dl, grad_out):
    plan = _vgg_plan(model)
    flat = model.classifier.weight._ddpx_flat
    cls = model.classifier
    xlast, feat = last
    dW, acc = flat.grad_target(cls.weight)
    db, _ = flat.grad_target(cls.bias)
    dfeat = F.head_backward(dl, grad_out, feat, cls.weight, dW, db, accumulate=acc)
    flat.grad_done(cls.weight)
    flat.grad_done(cls.bias)
    tail, scale = tail_of(model)
    g = F.gmaxpool_backward(dfeat, xlast, scale) if tail == "max" else F.avgpool_backward(dfeat, *xlast)
    comm = _sync_comm(model, True)
    # residual blocks: the gradient at an add's output goes to the branch and, unchanged, to the block the skip came
    # from, whose BatchNorm backward takes the pair (branch data gradient, skip gradient) without storing their sum
    skip_g = {}
    for bi in range(len(plan.blocks) - 1, -1, -1):
        conv, bn, pool = plan.blocks[bi]
        x, y, a, b, mean, rstd, (N, H, W, C, Co), wino = saved[bi]
        if plan.skip[bi] is not None:
            skip_g[plan.skip[bi]] = g
        dgam, accg = flat.grad_target(bn.weight)
        dbet, _ = flat.grad_target(bn.bias)
        dy = F.bn_backward(g, y, a, b, mean, rstd, N, H, W, Co, pool, dgam, dbet, accumulate=accg, comm=comm,
                           g2=skip_g.pop(bi, None))
        flat.grad_done(bn.weight)
        flat.grad_done(bn.bias)
        _grad_write(flat, conv.weight, lambda o, ac: F.conv_wgrad(dy, x, Co, conv.weight.shape[1], o, ac))
        if bi > 0:
            g = plan.dgrad(bi, dy, N, H, W, C, Co, wino)


VGG_GRAPH = Graph(lambda model, x, targets, soft, for_loss: _vgg_forward(model, x, targets, model.training, soft),
                  _vgg_backward)


def vgg_loss(model, x, targets, soft=None):
    return LossNode.apply(VGG_GRAPH, prep_vgg_input(x), targets, model, soft, *model.parameters())


def vgg_logits(model, x):
    """Inference logits (no autograd through the native fp32 path)."""
    with torch.no_grad():
        _, _, _, logits, _ = _vgg_forward(model, prep_vgg_input(x), None, model.training)
    return logits


# ddpx/models/resnet.py on VGG's graph (the plan carries the skip connections): the add in the BatchNorm apply pass,
# the two gradients that meet below a residual block summed inside the BatchNorm backward kernels.
resnet_loss = vgg_loss


def resnet_forward(model, x):
    """Logits: plain under ``no_grad``, through an autograd node otherwise."""
    if not torch.is_grad_enabled():
        return vgg_logits(model, x)
    return LogitsNode.apply(VGG_GRAPH, prep_vgg_input(x), model, *model.parameters())


# ---------------------------------------------------------------------------------------------- DeepNN
# /root/reference/singlegpu.py:18-44 at the reference's precision: [conv3x3+bias -> ReLU] x2 -> MaxPool2 ->
# [conv3x3+bias -> ReLU] x2 -> MaxPool2 -> flatten (C,H,W) -> Linear(2048,512) -> ReLU -> Dropout(0.1) ->
# Linear(512,10).  Conv bias + ReLU in the GEMM epilogue; the pool (and the backward's ReLU mask + first-max
# routing + bias gradient) through the BatchNorm kernels with the identity affine (a = 1, b = 0, mean = 0,
# rstd = 1, and c1 = c2 = 0 in the apply: dy = routed, masked gradient).
class _DeepNNPlan(DeepNNPlanBase, _ConvWeights):
    def __init__(self, model):
        DeepNNPlanBase.__init__(self, model)
        dev = self.lin0.weight.device
        # Winograd F(2,3) forward (+ bias + ReLU epilogue) and data gradient where it applies (the 128 -> 64,
        # 64 -> 64 and 64 -> 32 layers), the direct implicit GEMM elsewhere
        _ConvWeights.__init__(self, self.blocks, dev, lazy_direct=False)
        self.scratch = torch.empty(2 * self.ones.numel(), dtype=torch.float32, device=dev)


def _deepnn_plan(model):
    return plan_of(model, "_ddpx_plan_f32", _DeepNNPlan)


def _deepnn_forward(model, x, targets, training, soft=None):
    plan = _deepnn_plan(model)
    saved = []
    N, H, W, C = x.shape
    for bi, (conv, pool) in enumerate(plan.blocks):
        Co = conv.weight.shape[0]
        P = N * H * W
        wino = plan.prep(bi, conv, x)
        if wino:
            y = F.wino_conv(x, plan.uf[bi], Co, bias=conv.bias, relu=True)
        else:
            y = torch.empty((P, Co), dtype=torch.float32, device=x.device)
            F.gemm(F.IM2COL_KC, x, 0, F.DENSE_OC, plan.wf[bi], Co, P, Co, 9 * C, y, geom=(C, H, W, 1),
                   bias=conv.bias, relu=True)
        # the pool alone: the BatchNorm apply pass with the identity affine (a = 1, b = 0, mean = 0)
        xn = F.bn_apply(y, plan.ones, plan.zeros, plan.zeros, N, H, W, Co, True) if pool else y.view(N, H, W, Co)
        saved.append((x, y, (N, H, W, C, Co), pool, wino))
        x = xn
        H, W, C = xn.shape[1], xn.shape[2], Co
    feat = F.nchw_flatten(x)
    l0, l1 = plan.lin0, plan.lin1
    a0 = F.linear_fwd(feat, l0.weight, l0.bias, relu=True)
    p = float(plan.drop.p)
    drop = training and p > 0.0
    d0 = F.dropout_(a0, p, plan.rng, plan.rng_done) if drop else a0
    loss, logits, dl = F.head_forward(d0, l1.weight, l1.bias, targets, soft)
    scale = 1.0 / (1.0 - p) if drop else 1.0
    return saved, (x.shape, feat, d0, scale), loss, logits, dl


def _deepnn_backward(model, saved, last, dl, grad_out):
    plan = _deepnn_plan(model)
    l0, l1 = plan.lin0, plan.lin1
    flat = l0.weight._ddpx_flat
    xshape, feat, d0, scale = last
    dW1, acc = flat.grad_target(l1.weight)
    db1, _ = flat.grad_target(l1.bias)
    # Dropout + ReLU backward folded into the head's dh: mask d0 > 0 (kept and positive), scale 1/(1-p)
    dd0 = F.head_backward(dl, grad_out, d0, l1.weight, dW1, db1, accumulate=acc, relu_mask=True, dh_scale=scale)
    flat.grad_done(l1.weight)
    flat.grad_done(l1.bias)
    _grad_write(flat, l0.bias, lambda o, ac: F.colsum(dd0, o, ac))
    _grad_write(flat, l0.weight, lambda o, ac: F.linear_wgrad(dd0, feat, o, ac))
    g = F.nchw_unflatten(F.linear_dgrad(dd0, l0.weight), *xshape)
    g_masked = False  # g already through the block's ReLU (the producing dgrad's epilogue applied the mask)
    for bi in range(len(plan.blocks) - 1, -1, -1):
        conv, pool = plan.blocks[bi]
        x, y, (N, H, W, C, Co), _, wino = saved[bi]
        dy = None

        def bias_grad(o, ac):
            nonlocal dy
            if g_masked:
                dy = g.reshape(N * H * W, Co)
                F.colsum_bias(dy, N * H * W, Co, plan, o, ac)
            else:
                dy = F.bias_act_backward(g, y, N, H, W, Co, pool, plan, o, ac)
        _grad_write(flat, conv.bias, bias_grad)
        _grad_write(flat, conv.weight, lambda o, ac: F.conv_wgrad(dy, x, Co, conv.weight.shape[1], o, ac))
        if bi > 0:
            # DDPX_F32_DGRAD_MASK: the Winograd data gradient applies the ReLU mask of a non-pooled block below
            g_masked = F._DGRAD_MASK and plan.wino_dgrad(bi, wino) and not plan.blocks[bi - 1][1]
            g = plan.dgrad(bi, dy, N, H, W, C, Co, wino, mask=saved[bi - 1][1] if g_masked else None)


DEEPNN_GRAPH = Graph(lambda model, x, targets, soft, for_loss:
                     _deepnn_forward(model, x, targets, model.training, soft), _deepnn_backward)


def deepnn_loss(model, x, targets, soft=None):
    return LossNode.apply(DEEPNN_GRAPH, prep_vgg_input(x), targets, model, soft, *model.parameters())


def deepnn_logits(model, x):
    with torch.no_grad():
        _, _, _, logits, _ = _deepnn_forward(model, prep_vgg_input(x), None, model.training)
    return logits


# ---------------------------------------------------------------------------------------------- MLP
def _mlp_forward(model, x, targets, soft=None):
    lins = model.linears()
    hs = [x]
    for lin in lins[:-1]:
        hs.append(F.linear_fwd(hs[-1], lin.weight, lin.bias, relu=True))
    last = lins[-1]
    loss, logits, dl = F.head_forward(hs[-1], last.weight, last.bias, targets, soft)
    return hs, loss, logits, dl


def _mlp_backward(model, hs, dl, grad_out):
    lins = model.linears()
    flat = lins[0].weight._ddpx_flat
    last = lins[-1]
    dW, acc = flat.grad_target(last.weight)
    db, _ = flat.grad_target(last.bias)
    dz = F.head_backward(dl, grad_out, hs[-1], last.weight, dW, db, accumulate=acc, relu_mask=True)
    flat.grad_done(last.weight)
    flat.grad_done(last.bias)
    for i in range(len(lins) - 2, -1, -1):
        lin = lins[i]
        sw = flat.fused_spec(lin.weight)
        if sw is not None:
            # single process, SGD(fused_backward): the data gradient reads W_i first, then the weight-gradient
            # GEMM updates W_i in its epilogue (no gradient stored, no separate optimizer pass over W_i)
            dz_next = F.linear_dgrad(dz, lin.weight, mask=hs[i]) if i > 0 else None
            if F.linear_wgrad_sgd(dz, hs[i], sw):
                flat.mark_updated(lin.weight)
            else:
                _grad_write(flat, lin.weight, lambda o, ac: F.linear_wgrad(dz, hs[i], o, ac))
            _grad_write(flat, lin.bias, lambda o, ac: F.colsum(dz, o, ac))
            if i > 0:
                flat.release(lin.weight)
                dz = dz_next
            continue
        _grad_write(flat, lin.weight, lambda o, ac: F.linear_wgrad(dz, hs[i], o, ac))
        _grad_write(flat, lin.bias, lambda o, ac: F.colsum(dz, o, ac))
        if i > 0:
            dz = F.linear_dgrad(dz, lin.weight, mask=hs[i])
            flat.release(lin.weight)  # last read of W_i in this backward


MLP_GRAPH = Graph(lambda model, x, targets, soft, for_loss: _mlp_forward(model, x, targets, soft), _mlp_backward)


def mlp_loss(model, x, targets, soft=None):
    x = x.reshape(x.shape[0], -1).float().contiguous()
    return LossNode.apply(MLP_GRAPH, x, targets, model, soft, *model.parameters())


def mlp_logits(model, x):
    with torch.no_grad():
        _, _, logits, _ = _mlp_forward(model, x.reshape(x.shape[0], -1).float().contiguous(), None)
    return logits
