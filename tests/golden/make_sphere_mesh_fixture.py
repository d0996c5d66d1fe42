"""Generator of tests/golden/sphere_mesh_500.npz: the triangle mesh behind tests/golden/sphere_phi_500x32.npz -- the 500
vertices and 996 faces of the reference's tests/sphere.obj (a Fibonacci sphere, written by the reference's
tests/generate_data_for_test_linalg.py), on which its test_linalg.c computes the 32 eigenpairs with lambda in [50, 100] of the
consistent-mass pencil.  The eigenvalues and vectors stay in sphere_phi_500x32.npz.  DATA only is copied (numbers), no
source text.

    python tests/golden/make_sphere_mesh_fixture.py <the reference's tests directory>
"""
import os
import sys

import numpy as np

REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))

lines = open(os.path.join(REF, "sphere.obj")).read().splitlines()
verts = np.array([[float(t) for t in ln.split()[1:4]] for ln in lines if ln.startswith("v ")])
faces = np.array([[int(t.split("/")[0]) - 1 for t in ln.split()[1:4]] for ln in lines if ln.startswith("f ")], dtype=np.uint64)
assert verts.shape == (500, 3) and faces.shape == (996, 3) and faces.max() == 499
assert np.allclose(np.linalg.norm(verts, axis=1), 1.0, atol=1e-12)
assert np.array_equal(verts, np.load(os.path.join(HERE, "sphere_phi_500x32.npz"))["points"])
# a closed surface of genus 0: every edge in two faces, V - E + F = 2
edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
uniq, counts = np.unique(edges, axis=0, return_counts=True)
assert (counts == 2).all() and 500 - len(uniq) + 996 == 2
np.savez_compressed(os.path.join(HERE, "sphere_mesh_500.npz"), verts=verts, faces=faces)
print("wrote sphere_mesh_500.npz", verts.shape, faces.shape)
