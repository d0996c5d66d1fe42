"""Eigenbands to the butterfly of Phi with the SVDs on the device (butterfly_amd/streamer_build.py):
the streaming pipeline through DeviceSvdFactorizer against the numpy-driven run of oracle/streamer_values.py (every SVD's
(m, n, k), the descriptor's structure, the operator against the dense Phi), and ChebCovariance.eigs_butterfly on the
committed sphere mesh against its own dense eigenvectors."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-3


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


@pytest.fixture(scope="module")
def pipeline():
    """sphere_lbo_problem(600, 11), freq_depth 2, tol 1e-3: 52 SVDs, rows 74-600, columns 27-209, 24 of them wide; the
    smallest relative distance of a singular value to its threshold is 8.4e-3, so k cannot hinge on rounding."""
    from butterfly_amd import streamer_build as sb, streamer_structure as ss
    from oracle import streamer_values as sv
    pts, phi, freqs = sv.sphere_lbo_problem(600, 11)
    wmax = float(np.sqrt(11 * 12.0) * 1.0001)
    rec = []
    st, a_phi = sv.stream_columns(pts, phi, freqs, wmax, 2, tol=TOL, record=rec)
    desc, vals = ss.to_desc(st.get_mat())
    op, perm, info = sb.stream_butterfly(pts, phi, freqs, wmax, freq_depth=2, tol=TOL, max_rhs=64, check_columns=8)
    yield dict(st=st, a_phi=a_phi, desc=desc, rec=rec, op=op, perm=perm, info=info, graph=st.get_mat())
    op.close()


def test_every_svd_keeps_the_count_of_the_numpy_run(pipeline):
    want = [(m, n, k) for m, n, _, _, k in pipeline["rec"]]
    got = [(m, n, k) for m, n, k, _, _ in pipeline["info"]["svd_records"]]
    print("sweeps per SVD:", sorted({s for *_, s, _ in pipeline["info"]["svd_records"]}), "svd seconds", pipeline["info"]["svd_seconds"],
          "host seconds", pipeline["info"]["host_seconds"])
    assert len(want) == 52 and got == want
    assert max(s for *_, s, _ in pipeline["info"]["svd_records"]) <= 30


def test_structure_is_the_numpy_runs(pipeline):
    d, e = pipeline["info"]["desc"], pipeline["desc"]
    assert d.root == e.root and d.kind == e.kind and d.rows == e.rows and d.cols == e.cols and d.block_kind == e.block_kind
    assert [[tuple(c) for c in ch] for ch in d.children] == [[tuple(c) for c in ch] for ch in e.children]
    assert {k: pipeline["info"][k] for k in ("svds", "merges", "feeds")} == pipeline["st"].stats


def test_operator_reproduces_phi_within_the_tolerance(pipeline):
    """64 columns of the identity give the matching columns of Phi in tree order, and the streamer's own acceptance check
    (src/fac_streamer.c:286-301) holds: relative Frobenius error <= tol.  The numpy-driven operator gives 3.7e-4 on random
    vectors; its figure on the same identity columns is printed beside the device's."""
    import torch
    from oracle import streamer_values as sv
    a_phi, op = pipeline["a_phi"], pipeline["op"]
    J = a_phi.shape[1]
    cols = np.linspace(0, J - 1, 64).astype(int)
    E = np.zeros((J, 64))
    E[cols, np.arange(64)] = 1.0
    got = op.apply_device(torch.from_numpy(E).cuda()).cpu().numpy()
    ref = np.stack([sv.apply(pipeline["graph"], E[:, q]) for q in range(64)], axis=1)
    print(f"identity columns: device-built {rel(got, a_phi[:, cols]):.3e}, numpy-built {rel(ref, a_phi[:, cols]):.3e}; "
          f"acceptance on random vectors {pipeline['info']['acceptance']:.3e}")
    assert rel(got, a_phi[:, cols]) <= TOL
    assert pipeline["info"]["acceptance"] <= TOL
    x = np.random.default_rng(3).standard_normal((J, 64))
    assert rel(op.apply_device(torch.from_numpy(x).cuda()).cpu().numpy(), a_phi @ x) <= TOL


def test_eigs_butterfly_on_the_committed_sphere_mesh():
    """The lowest 64 pairs of tests/golden/sphere_mesh_500.npz: the butterfly applied to 64 random w against the dense
    matmul with eigs_bands' own Phi, and cov_sample_block_device through the butterfly against Phi gamma(Lambda) w; both to the
    relative tolerance of the factorization."""
    import torch
    from butterfly_amd import ChebCovariance
    mesh = np.load(os.path.join(HERE, "golden", "sphere_mesh_500.npz"))
    cov = ChebCovariance.from_trimesh(mesh["verts"], mesh["faces"])
    op, perm, lam, info = cov.eigs_butterfly(mesh["verts"], 64, band=32, tol=TOL, return_info=True, max_rhs=64)
    phi = info["phi"]
    assert op.shape == (500, 64) and lam.shape == (64,) and np.all(np.diff(lam) >= 0) and perm.dtype == torch.int64 and perm.is_cuda
    assert sorted(perm.cpu().tolist()) == list(range(500))
    w = torch.from_numpy(np.random.default_rng(7).standard_normal((64, 64))).cuda()
    dense = phi.contiguous() @ w
    got = torch.empty_like(dense)
    got[perm] = op.apply_device(w)                      # the operator's rows are in tree order
    e1 = float(torch.linalg.norm(got - dense) / torch.linalg.norm(dense))
    gam = torch.from_numpy(1.0 / (1.0 + lam)).cuda()
    z = op.cov_sample_block_device(gam, perm, w)
    want = phi.contiguous() @ (gam[:, None] * w)
    e2 = float(torch.linalg.norm(z - want) / torch.linalg.norm(want))
    print(f"eigs_butterfly: apply {e1:.3e}, sample {e2:.3e}, svds {info['svds']}, freq_depth {info['freq_depth']}")
    assert e1 <= TOL and e2 <= TOL
    op.close()
    cov.close()
