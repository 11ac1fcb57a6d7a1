"""Host side of the row-pass skipping (functional.ROW_SKIP_DROPPED): the predicate that decides whether a branch's
stochastic-depth factor may travel to the backward row kernels, and the one-slot holder through which the branch's first
GEMM hands it back to the node that produced its normalised input.  No GPU: the factor is a stand-in object."""
import pytest
import torch


class _Scale:
    """What row_skip_scale looks at, with a CUDA tensor's answers."""

    def __init__(self, n, is_cuda=True, dtype=torch.float32, dim=1, contiguous=True):
        self.n, self.is_cuda, self.dtype, self._dim, self._c = n, is_cuda, dtype, dim, contiguous

    def dim(self):
        return self._dim

    def is_contiguous(self):
        return self._c

    def numel(self):
        return self.n

    def detach(self):
        return self


@pytest.fixture
def OF():
    import octic_vits_amd.functional as OF
    before = OF.ROW_SKIP_DROPPED
    OF.ROW_SKIP_DROPPED = True
    yield OF
    OF.ROW_SKIP_DROPPED = before


def test_the_predicate_is_that_of_the_weight_gradient_skip(OF):
    rs = _Scale(8)
    assert OF.row_skip_scale(rs, 257, 8 * 257) is rs
    assert OF.row_skip_scale(None, 257, 8 * 257) is None                       # eval, drop_path 0
    assert OF.row_skip_scale(rs, 257, 8 * 257, rows_to=object()) is None       # compact rows of a stream
    assert OF.row_skip_scale(rs, 1, 8) is None                                 # per-row factors of a ragged row tensor
    assert OF.row_skip_scale(rs, 257, 8 * 257 + 1) is None                     # not whole samples
    assert OF.row_skip_scale(_Scale(8, is_cuda=False), 257, 8 * 257) is None
    assert OF.row_skip_scale(_Scale(8, dtype=torch.bfloat16), 257, 8 * 257) is None
    assert OF.row_skip_scale(_Scale(8, dim=2), 257, 8 * 257) is None
    assert OF.row_skip_scale(_Scale(8, contiguous=False), 257, 8 * 257) is None
    OF.ROW_SKIP_DROPPED = False
    assert OF.row_skip_scale(rs, 257, 8 * 257) is None
    # the same answers as wgrad_skip_scale, argument for argument
    OF.ROW_SKIP_DROPPED = True
    before = OF.WGRAD_SKIP_DROPPED
    try:
        OF.WGRAD_SKIP_DROPPED = True
        for args in ((rs, 257, 2056), (rs, 1, 8), (rs, 257, 2057), (_Scale(8, False), 257, 2056), (None, 257, 2056),
                     (_Scale(8, dim=2), 257, 2056), (rs, 257, 2056, object())):
            assert (OF.row_skip_scale(*args) is None) == (OF.wgrad_skip_scale(*args) is None), args
    finally:
        OF.WGRAD_SKIP_DROPPED = before


def test_the_switch_reads_the_environment(monkeypatch):
    import octic_vits_amd.functional as OF
    monkeypatch.delenv("OCTIC_ROW_SKIP", raising=False)
    assert OF._skip_from_env("OCTIC_ROW_SKIP") is True
    monkeypatch.setenv("OCTIC_ROW_SKIP", "0")
    assert OF._skip_from_env("OCTIC_ROW_SKIP") is False
    monkeypatch.setenv("OCTIC_ROW_SKIP", " 1 ")
    assert OF._skip_from_env("OCTIC_ROW_SKIP") is True


class _Ctx:
    pass


def test_the_slot_hands_one_factor_back(OF):
    rs = _Scale(8)
    ctx, yn = _Ctx(), torch.zeros(2, 3)
    assert OF.row_skip_get(ctx, 2056) == (None, 0)                             # a producer without a slot
    OF.row_skip_attach(ctx, yn)
    assert yn._octic_row_skip is ctx.row_skip
    assert OF.row_skip_get(ctx, 2056) == (None, 0)                             # nobody filled it: no mask
    OF.row_skip_fill(yn, rs, 257, 2056)
    assert OF.row_skip_get(ctx, 2056) == (rs, 257)
    assert OF.row_skip_get(ctx, 2057) == (None, 0)                             # another row count than the consumer saw
    OF.row_skip_fill(yn, rs, 257, 2056)                                        # a second reader: cotangents are summed
    assert OF.row_skip_get(ctx, 2056) == (None, 0)


def test_a_consumer_without_a_factor_leaves_no_mask(OF):
    ctx, yn = _Ctx(), torch.zeros(2, 3)
    OF.row_skip_attach(ctx, yn)
    OF.row_skip_fill(yn, None, 257, 2056)
    assert OF.row_skip_get(ctx, 2056) == (None, 0)
    OF.row_skip_fill(torch.zeros(1), _Scale(8), 257, 2056)                     # a tensor no producer marked: nothing happens
    fresh = _Ctx()
    OF.row_skip_attach(fresh, yn)                                              # the next forward: a fresh slot
    assert OF.row_skip_get(fresh, 2056) == (None, 0) and OF.row_skip_get(ctx, 2056) == (None, 0)


def test_the_slot_travels_through_an_autograd_node(OF):
    """Attached inside a Function.forward, found by the consumer's forward, read in the producer's backward."""
    seen = []

    class Producer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            yn = (x * 2).view(x.shape)
            OF.row_skip_attach(ctx, yn)
            return x.view_as(x), yn

        @staticmethod
        def backward(ctx, g0, g1):
            seen.append(OF.row_skip_get(ctx, 4))
            return g1 * 2

    class Consumer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, rs):
            OF.row_skip_fill(x, rs, 2, 4)
            return x * 3

        @staticmethod
        def backward(ctx, g):
            return g * 3, None

    rs = _Scale(2)
    x = torch.ones(4, requires_grad=True)
    _, yn = Producer.apply(x)
    Consumer.apply(yn, rs).sum().backward()
    assert seen == [(rs, 2)]
