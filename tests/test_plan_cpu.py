"""The model walks the native graphs of both precisions share (``ddpx.ops.plan``) and the plans built on them, for
CPU models: block structure, skip tables and the sizes of the prepared-weight buffers."""
import torch
from torch import nn

from ddpx.models import VGG, DeepNN
from ddpx.models.resnet import ResNet9
from ddpx.ops import conv as K
from ddpx.ops import deepnn_native, f32, f32_native, vgg_native
from ddpx.ops.plan import conv_blocks, deepnn_blocks


def test_conv_blocks_vgg():
    m = VGG()
    blocks, skip = conv_blocks(m)
    assert len(blocks) == 8 and skip == [None] * 8
    assert [bi for bi, (_, _, pool) in enumerate(blocks) if pool] == [1, 3, 5, 7]
    for bi, (conv, bn, _) in enumerate(blocks):
        assert conv is getattr(m.backbone, f"conv{bi}") and bn is getattr(m.backbone, f"bn{bi}")


def test_conv_blocks_resnet9():
    m = ResNet9()
    blocks, skip = conv_blocks(m)
    nb = m.native_blocks()
    assert len(blocks) == len(skip) == len(nb) == 8
    for (conv, bn, pool), k, (nconv, nbn, npool, nk) in zip(blocks, skip, nb):
        assert conv is nconv and bn is nbn and pool == npool and k == nk
    assert skip == [None, None, None, 1, None, None, None, 5]
    for plan in (vgg_native._Plan(m), f32_native._VGGPlan(m)):
        assert plan.skip == skip and plan.skipped == {k for k in skip if k is not None} == {1, 5}
    for plan in (vgg_native._Plan(VGG()), f32_native._VGGPlan(VGG())):
        assert plan.skipped == set()


def test_deepnn_blocks():
    m = DeepNN()
    blocks, lin0, drop, lin1 = deepnn_blocks(m)
    assert len(blocks) == 4 and [bi for bi, (_, pool) in enumerate(blocks) if pool] == [1, 3]
    assert [c for c, _ in blocks] == [mod for mod in m.features if isinstance(mod, nn.Conv2d)]
    assert lin0 is m.classifier[0] and drop is m.classifier[2] and lin1 is m.classifier[3]


def _convs(plan):
    return [blk[0] for blk in plan.blocks]


def test_bf16_plan_buffers():
    """wf and wd of every 3x3 convolution: Co * 9 * padded_channels(Ci) bf16 elements each."""
    for plan in (vgg_native._Plan(VGG()), vgg_native._Plan(ResNet9()), deepnn_native._Plan(DeepNN())):
        convs = _convs(plan)
        assert len(plan.wf) == len(plan.wd) == len(convs) and plan.wver == [None] * len(convs)
        for conv, wf, wd in zip(convs, plan.wf, plan.wd):
            Co, Ci = conv.weight.shape[:2]
            assert wf.numel() == wd.numel() == Co * 9 * K.padded_channels(Ci)
            assert wf.dtype == wd.dtype == torch.bfloat16


def test_f32_plan_buffers_on_cpu():
    """On the CPU no layer is planned for Winograd, so both networks hold the direct layouts alone: wf of
    9 * Cp * Co elements, wd of 9 * Co * Ci where the direct data gradient takes the channel count (Ci % 4 == 0)."""
    for plan in (f32_native._VGGPlan(VGG()), f32_native._VGGPlan(ResNet9()), f32_native._DeepNNPlan(DeepNN())):
        convs = _convs(plan)
        assert len(plan.wf) == len(plan.wd) == len(plan.uf) == len(plan.ud) == len(convs)
        assert plan.uf == [None] * len(convs) and plan.ud == [None] * len(convs)
        for conv, wf, wd in zip(convs, plan.wf, plan.wd):
            Co, Ci = conv.weight.shape[:2]
            assert wf.dtype == torch.float32 and wf.numel() == 9 * f32.conv_channels(Ci) * Co
            if Ci % 4 == 0:
                assert wd.dtype == torch.float32 and wd.numel() == 9 * Co * Ci
            else:
                assert wd is None


def test_deepnn_plans_share_their_state():
    """ones / zeros over the widest layer and the dropout state, in both precisions; the fp32 plan adds scratch."""
    for plan in (deepnn_native._Plan(DeepNN()), f32_native._DeepNNPlan(DeepNN())):
        assert torch.equal(plan.ones, torch.ones(128)) and torch.equal(plan.zeros, torch.zeros(128))
        assert plan.rng.dtype == torch.int64 and plan.rng.shape == (2,) and int(plan.rng[1]) == 0
        assert 0 <= int(plan.rng[0]) < 2 ** 62
        assert plan.rng_done.dtype == torch.int32 and int(plan.rng_done[0]) == 0
        assert isinstance(plan.drop, nn.Dropout) and plan.lin0.out_features == 512
    assert f32_native._DeepNNPlan(DeepNN()).scratch.numel() == 2 * 128
