"""The classifier tail of the INT8 nets as its two launches run it (cases and seeded inputs: tests/tail_util.py):

  * 1x1 conv 512 -> 2048 (+ eltwise) + global average pooling (conv1x1_gpool.hip behind set_global_pooling / dispatch_gpool): the conv's
    bytes and the pooled bytes are the oracle's, the pooled bytes are those of the INT8 pooling op on y, for image sizes that leave
    pixel slots empty, fill all 64, fill less than one 16-pixel fragment or hold one pixel, batches 1 / 3 / 8, a channel count that is
    no multiple of the workgroup's 64, and all four epilogue forms - three launches in a row on changing inputs;
  * fc + Softmax in one launch (fc_small.hip, 512 threads): logits are fc.dispatch's bits, prob is BIT FOR BIT what the parent
    commit's four-wave form wrote for the same seeded inputs (tests/golden/fc_softmax_tail.npz, recorded once on the GPU by
    scripts/record_fc_softmax_golden.py with a built copy of the parent) - the eight-wave tail keeps the lane <-> column map, the
    order of the row sum, expf and the division - then 12 launches on changing inputs under the fused launch's usual criteria."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from anakin_amd import lib as L  # noqa: E402
from anakin_amd import saber as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import tail_util as T  # noqa: E402

FP32_RTOL = 1e-4      # tests/test_gpu_parity.py


@pytest.fixture(scope="module", autouse=True)
def _device():
    L.require_device()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("epi", T.GPOOL_EPILOGUES, ids=[e[0] for e in T.GPOOL_EPILOGUES])
@pytest.mark.parametrize("cout", T.GPOOL_COUTS)
@pytest.mark.parametrize("N", T.GPOOL_BATCHES)
@pytest.mark.parametrize("H,W", T.GPOOL_IMAGES)
def test_conv1x1_with_global_pooling_equals_oracle(H, W, N, cout, epi):
    wq, ws, b, xs, rs = T.gpool_case(H, W, N, cout, epi)
    elt = epi[1]
    conv = T.gpool_op(N, H, W, cout, wq, ws, b, epi)
    assert conv.algo() == "imgres1x1_i8_64ch+gpool", conv.algo()
    y = conv.new_output()
    yp = torch.empty((N, 1, 1, cout), dtype=y.dtype, device="cuda")
    for it in range(T.GPOOL_LAUNCHES):
        want, want_pool = T.gpool_oracle(wq, ws, b, xs[it], rs[it], epi)
        y.fill_(77)
        yp.fill_(55)
        conv.dispatch_gpool(dev(xs[it]), y, yp, dev(rs[it]) if elt else None)
        got, got_pool = host(y), host(yp)
        assert got.dtype == want.dtype and np.array_equal(got, want), (it, conv.algo())
        assert got_pool.dtype == want_pool.dtype and np.array_equal(got_pool, want_pool), (it, conv.algo())
        pool = S.pooling_i8(y, (H, W), (1, 1), (0, 0), 1, global_pooling=True)
        assert np.array_equal(host(pool).reshape(got_pool.shape), got_pool), it


@pytest.fixture(scope="module")
def golden():
    return np.load(T.GOLDEN)


@pytest.mark.parametrize("case", T.FC_CASES, ids=[T.fc_key(c) for c in T.FC_CASES])
def test_fc_softmax_logits_exact_and_prob_bits_of_the_parent(case, golden):
    M, K, N, dt = case
    wq, ws, b, out_scale, xs = T.fc_case(case)
    fc = T.fc_op(case, wq, ws, b, out_scale)
    assert fc.algo() == "fc_i8_small_16xk4", fc.algo()
    y = torch.empty((M, N), dtype=torch.float32, device="cuda")
    p = torch.empty((M, N), dtype=torch.float32, device="cuda")
    y2 = torch.empty((M, N), dtype=torch.float32, device="cuda")
    key = T.fc_key(case)
    assert golden[key + "/inputs"] == T.fingerprint(wq, ws, b, xs[0]), "the golden file was recorded for other inputs"
    for it in range(T.FC_LAUNCHES):
        xd = dev(xs[it])
        y.fill_(7.0)
        p.fill_(-1.0)
        fc.dispatch_softmax(xd, y, p)
        got_y, got_p = host(y), host(p)
        fc.dispatch(xd, y2)
        assert np.array_equal(got_y.view(np.uint32), host(y2).view(np.uint32)), (case, it)
        want = T.fc_oracle(case, wq, ws, b, out_scale, xs[it])
        assert np.array_equal(got_y, want), (case, it)
        sm = O.softmax_f32(want)
        assert np.abs(got_p - sm).max() <= FP32_RTOL * sm.max(), (case, it, np.abs(got_p - sm).max())
        assert np.allclose(got_p.sum(1), 1.0, atol=1e-5), (case, it)
        if it == 0:
            want_p = golden[key + "/prob"]
            assert want_p.shape == got_p.shape and want_p.dtype == np.float32
            diff = got_p.view(np.uint32) != want_p.view(np.uint32)
            assert not diff.any(), (case, int(diff.sum()), "of", diff.size, "prob words differ from the parent's")
