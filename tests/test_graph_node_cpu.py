"""The autograd node pair of the native model graphs (``ddpx.ops.graph_node``) on a fake graph over CPU tensors that
records its calls: what the nodes hand to the graph, what they return to autograd, and that they let go of the saved
state after the backward."""
import gc
import weakref

import pytest
import torch

from ddpx.ops.graph_node import Graph, LogitsNode, LossNode


class _FakeGraph:
    """forward -> (saved, last, loss, logits, dl) with two state items; every call is recorded."""

    def __init__(self):
        self.forward_calls, self.backward_calls = [], []
        self.state_ref = None
        self.graph = Graph(self.forward, self.backward)

    def forward(self, model, x, targets, soft, for_loss):
        self.forward_calls.append((model, x, targets, soft, for_loss))
        assert not torch.is_grad_enabled()  # inside the node: the graph's own ops build no autograd graph
        held = x * 2.0  # a tensor that only the saved state holds
        self.state_ref = weakref.ref(held)
        loss = x.sum() * 3.0
        logits = x[:, :3].double()  # non-fp32 logits, so that a non-fp32 gradient reaches the node
        dl = torch.full((2, 3), 0.5)
        return [held], ("last", 7), loss, logits, dl

    def backward(self, model, saved, last, dl, grad_out):
        self.backward_calls.append((model, saved, last, dl, grad_out))


def _params(n):
    return [torch.nn.Parameter(torch.randn(3)) for _ in range(n)]


@pytest.mark.parametrize("n", [0, 1, 4])
def test_loss_node(n):
    fake, model, params = _FakeGraph(), object(), _params(n)
    x = torch.randn(2, 5, requires_grad=(n == 0))  # with no parameter, the input makes the loss require grad
    targets, soft = torch.tensor([1, 0]), object()
    loss = LossNode.apply(fake.graph, x, targets, model, soft, *params)
    assert torch.equal(loss, x.detach().sum() * 3.0) and loss.requires_grad
    (call,) = fake.forward_calls
    assert call[0] is model and call[1] is x and call[2] is targets and call[3] is soft and call[4] is True
    assert fake.state_ref() is not None and not fake.backward_calls
    grad = torch.tensor(0.25)
    loss.backward(grad)  # autograd rejects a backward that returns another number of gradients than inputs
    (call,) = fake.backward_calls
    assert call[0] is model and call[2] == ("last", 7)
    assert torch.equal(call[1][0], x.detach() * 2.0)
    assert torch.equal(call[3], torch.full((2, 3), 0.5))
    assert torch.equal(call[4], grad)
    assert x.grad is None and all(p.grad is None for p in params)
    # the node (alive through loss.grad_fn) dropped what it saved; only the recorded call still holds it
    fake.backward_calls.clear()
    del call
    gc.collect()
    assert loss.grad_fn is not None and fake.state_ref() is None


@pytest.mark.parametrize("n", [0, 1, 4])
def test_logits_node(n):
    fake, model, params = _FakeGraph(), object(), _params(n)
    x = torch.randn(2, 5, requires_grad=(n == 0))
    logits = LogitsNode.apply(fake.graph, x, model, *params)
    assert torch.equal(logits, x.detach()[:, :3].double()) and logits.requires_grad
    (call,) = fake.forward_calls
    assert call[0] is model and call[1] is x and call[2] is None and call[3] is None and call[4] is False
    # a non-contiguous, non-fp32 gradient of the logits
    g = torch.randn(3, 2, dtype=torch.float64).t()
    assert not g.is_contiguous()
    logits.backward(g)
    (call,) = fake.backward_calls
    dl, grad_out = call[3], call[4]
    assert grad_out is None
    assert dl.dtype == torch.float32 and dl.is_contiguous() and torch.equal(dl, g.float())
    assert call[0] is model and call[2] == ("last", 7) and torch.equal(call[1][0], x.detach() * 2.0)
    assert x.grad is None and all(p.grad is None for p in params)
    fake.backward_calls.clear()
    del call
    gc.collect()
    assert logits.grad_fn is not None and fake.state_ref() is None


def test_state_of_any_length():
    """The graph's state is whatever precedes (loss, logits, dl): one item (the fp32 MLP) works as two do."""
    calls = []
    graph = Graph(lambda model, x, targets, soft, for_loss: (["hs"], x.sum(), None, "dl"),
                  lambda *a: calls.append(a))
    p = torch.nn.Parameter(torch.zeros(1))
    LossNode.apply(graph, torch.ones(2), None, "model", None, p).backward()
    (call,) = calls
    assert call[:3] == ("model", ["hs"], "dl") and torch.equal(call[3], torch.tensor(1.0))
