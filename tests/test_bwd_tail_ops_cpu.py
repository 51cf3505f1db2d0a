"""CPU path of the fused backward-tail ops: the composition of the plain
ops, with the bias gradient accumulated into db."""

import torch

from poseidon_amd.ops import functional as ops

K, S, P = (3, 3), (2, 2), (0, 0)


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_tail_ops_compose_on_cpu():
    x = torch.relu(_rnd(2, 8, 7, 7, seed=1))
    y, sc = ops.lrn_forward(x, 3, 1.0, 0.75)
    ypool, mask = ops.pool_max_forward(y, K, S, P)
    dpool = _rnd(*ypool.shape, seed=2)
    base = _rnd(8, seed=3)

    dnorm = ops.pool_max_backward(dpool, mask, x.shape, K, S, P)
    want = ops.relu_backward(x, ops.lrn_backward(x, y, sc, dnorm, 3, 1.0, 0.75))
    db = base.clone()
    got = ops.lrn_backward_tail(x, y, dpool, 3, 1.0, 0.75, relu=True, db=db,
                                pool=(mask, K, S, P))
    assert torch.equal(got, want)
    assert torch.allclose(db, base + want.sum(dim=(0, 2, 3)))

    _, xmask = ops.pool_max_forward(x, K, S, P)
    want = ops.relu_backward(
        x, ops.pool_max_backward(dpool, xmask, x.shape, K, S, P))
    db = base.clone()
    got = ops.pool_max_backward_tail(dpool, xmask, x, K, S, P, db=db)
    assert torch.equal(got, want)
    assert torch.allclose(db, base + want.sum(dim=(0, 2, 3)))

    dy = _rnd(2, 8, 7, 7, seed=4)
    want = ops.relu_backward(x, dy)
    db = base.clone()
    got = ops.relu_backward_bias(x, dy, db)
    assert torch.equal(got, want)
    assert torch.allclose(db, base + want.sum(dim=(0, 2, 3)))
