"""Derive the elasticity3Dbunny mesh fixtures from the reference's own data file.

    python tests/golden/make_bunny_fixture.py [path/to/reference]   # needs the reference checkout

The reference's elasticity/data/bunny.mesh (MEDIT ASCII, the mesh scripts/elasticity3Dbunny.sh
trains on) is not part of this repository; its vertices, tetrahedra and surface triangles are, as data:
tests/golden/bunny_mesh.npz = {V: (nv, 3) float64 as read, T: (nt, 4) int32 0-based},
tests/golden/bunny_faces.npz = {F: (nf, 3) int32 0-based, the file's Triangles block}.
pde/mesh.py load_mesh() reads bunny_mesh.npz as it reads the .mesh (normalise x2, boundary faces);
tests/test_mesh.py writes the three blocks back as a MEDIT file and reads that.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", "insr-pde_amd")]
from pde.mesh import read_medit  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("INSR_REFERENCE", "reference")
SRC = os.path.join(REF, "elasticity", "data", "bunny.mesh")


def main():
    V, blocks = read_medit(SRC)
    T = blocks["Tetrahedra"].astype(np.int32)
    F = blocks["Triangles"].astype(np.int32)
    out = os.path.join(HERE, "bunny_mesh.npz")
    np.savez_compressed(out, V=V, T=T)
    print(out, V.shape, T.shape, os.path.getsize(out))
    out = os.path.join(HERE, "bunny_faces.npz")
    np.savez_compressed(out, F=F)
    print(out, F.shape, os.path.getsize(out))


if __name__ == "__main__":
    main()
