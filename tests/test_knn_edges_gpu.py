"""-m gpu: csrc/knn.hip on directed clouds (tests/knn_ref.py) at sizes around its 1024-point boxes, against a brute force in the kernel's
own float32 formula.  What the clouds reach that one origin-centred Gaussian cloud does not: the zero-initialised bounding box that squeezes
the Morton codes of a cloud on one side of the origin, the degenerate axis (max - min == 0: NaN, code 0), duplicates (the pruning distance
`reject` is 0), pruning across distant clusters, and exactly tied distances."""
import numpy as np
import pytest
import torch

import knn_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", knn_ref.SIZES)
@pytest.mark.parametrize("kind", knn_ref.CLOUDS)
def test_knn_on_directed_clouds(kind, P):
    from gaussian_lic_amd import knn
    pts = knn_ref.cloud(kind, P)
    got = knn.distCUDA2(torch.from_numpy(pts).to("cuda:0")).cpu().numpy()
    ref32 = knn_ref.mean_dist2_f32(pts)
    assert got.shape == (P,) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    worst = int(np.argmax(err - 1e-6 * ref32))
    print(f"{kind} P={P}: max |got - ref32| / ref32 = {np.max(err / np.maximum(ref32, 1e-30)):.3e}, zeros {int((ref32 == 0).sum())}")
    # a squared distance is a sum of three non-negative products: fused or not it is within 2 ulp, and the mean adds three roundings — under
    # 6e-7 in all; the float32 selection can differ from the kernel's only among values that close
    assert (err <= 1e-6 * ref32).all(), (worst, got[worst], ref32[worst])
    assert (got[ref32 == 0] == 0).all()
    if kind == "four-times":
        assert (ref32 == 0).all() and (got == 0).all()
    if kind == "gaussian":
        assert rel_err(got, knn_ref.mean_dist2_f64(pts)) < 1e-5
