"""2-D affine transforms on homogeneous 3 x 3 matrices (the subset of the reference's functions/transform.py that step 10 uses).

A transform maps column vectors: ``[x', y', 1]^T = M [x, y, 1]^T``; ``transform`` takes points as rows ``(N, 2)``.  The builder
methods (``translation``, ``scaling``, ``rotation``, ``rotate_around``) compose IN PLACE and apply the new step AFTER the ones already
in the matrix (``M <- S M``), and return ``self`` so that they chain; ``A @ B`` is the matrix product (apply B first, then A)."""
import numpy as np


def _pair(v):
    if np.isscalar(v):
        return float(v), float(v)
    a, b = v
    return float(a), float(b)


class Affine:
    def __init__(self, matrix=None):
        if matrix is None:
            self.matrix = np.eye(3)
        else:
            m = np.asarray(matrix, dtype=np.float64)
            if m.shape != (3, 3):
                raise ValueError('an affine matrix is 3 x 3')
            self.matrix = m.copy()

    def __repr__(self):  # noqa
        return f'Affine({self.matrix!r})'

    def _then(self, step):
        self.matrix = step @ self.matrix
        return self

    def translation(self, offset):
        tx, ty = _pair(offset)
        return self._then(np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]]))

    def scaling(self, scale):
        sx, sy = _pair(scale)
        return self._then(np.array([[sx, 0.0, 0.0], [0.0, sy, 0.0], [0.0, 0.0, 1.0]]))

    def rotation(self, angle):
        """Counter-clockwise rotation by ``angle`` degrees about the origin."""
        r = np.deg2rad(angle)
        c, s = np.cos(r), np.sin(r)
        return self._then(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]))

    def rotate_around(self, angle, origin=(0, 0)):
        """Rotation by ``angle`` degrees about ``origin``: move the origin to 0, rotate, move back."""
        ox, oy = _pair(origin)
        self.translation((-ox, -oy))
        if angle != 0:
            self.rotation(angle)
        return self.translation((ox, oy))

    def inverse(self):
        """The inverse transform (a new object): linear part inverted, offset -A^-1 t."""
        a = np.linalg.inv(self.matrix[:2, :2])
        t = self.matrix[:2, 2]
        m = np.eye(3)
        m[:2, :2] = a
        m[0, 2] = -t[0] * a[0, 0] - t[1] * a[0, 1]
        m[1, 2] = -t[0] * a[1, 0] - t[1] * a[1, 1]
        return Affine(m)

    def transform(self, points):
        """Map points ``(N, 2)`` (or one point) to ``(N, 2)``."""
        p = np.atleast_2d(np.asarray(points, dtype=np.float64))
        ph = np.hstack((p, np.ones((p.shape[0], 1))))
        return (ph @ self.matrix.T)[:, :2]

    def __matmul__(self, other):
        if isinstance(other, Affine):
            return Affine(self.matrix @ other.matrix)
        return Affine(self.matrix @ np.asarray(other, dtype=np.float64))
