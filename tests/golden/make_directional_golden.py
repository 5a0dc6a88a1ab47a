"""Regenerates ref_directional_codebook_16x16_packed.npz from the reference's directional codebook.

    python tests/golden/make_directional_golden.py <reference root>

codebook/codebook_mat/directional_codebook_16x16.mat holds ``cb``, 32 x 32 x 256 complex: the 2-bit phase codes of
the 32 x 32 directional beam pairs main.py measures before its random probing (main/main.py:222), every entry in
{1, j, -1, -j}.  The fixture stores the codes k (entry j^k) four per byte along the last axis (code of element c in
bits 2 (c % 4) of byte c // 4), as ref_codebooks_16x16_packed.npz does, and their SHA-256.  Data only.
"""
import hashlib
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
NAME = "ref_directional_codebook_16x16_packed.npz"


def unpack(path=HERE / NAME):
    """The codebook of the fixture: cb [32][32][256] complex128, exact powers of j."""
    g = np.load(path)
    p = g["directional"]
    k = np.stack([(p >> (2 * i)) & 3 for i in range(4)], axis=-1).reshape(p.shape[0], p.shape[1], -1)
    assert hashlib.sha256(np.ascontiguousarray(k.astype(np.uint8)).tobytes()).hexdigest() == str(g["directional_sha256"])
    return np.array([1.0, 1j, -1.0, -1j])[k]


def main(root):
    import scipy.io as sio
    mat = pathlib.Path(root) / "codebook" / "codebook_mat" / "directional_codebook_16x16.mat"
    cb = sio.loadmat(str(mat))["cb"]   # plain MATLAB v5 numeric array, no pickle
    assert cb.shape == (32, 32, 256), cb.shape
    k = np.rint(np.angle(cb) / (np.pi / 2)).astype(np.int64) % 4
    assert np.allclose(1j ** k, cb, atol=1e-12), "directional codebook entries are not unit QPSK"
    k = k.astype(np.uint8)
    digest = hashlib.sha256(np.ascontiguousarray(k).tobytes()).hexdigest()
    q = k.reshape(32, 32, 64, 4)
    packed = (q[..., 0] | (q[..., 1] << 2) | (q[..., 2] << 4) | (q[..., 3] << 6)).astype(np.uint8)
    np.savez_compressed(HERE / NAME, directional=packed, directional_sha256=np.array(digest))
    assert np.array_equal(unpack(), np.array([1.0, 1j, -1.0, -1j])[k])
    print("directional codebook packed", packed.shape, digest[:16])


if __name__ == "__main__":
    main(sys.argv[1])
