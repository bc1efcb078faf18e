"""2x2 block matrices with diagonal blocks: the operators of a homogeneous medium (half-spaces, homogeneous layers) in O(N) instead of n^3."""
import torch


class BlockDiag2:
    """2x2 block matrix whose four N x N blocks are diagonal (Vf, Vi, Vo, Sin, Sout all have this form,
    rcwa.py:1143-1181): stored as four [B,N] diagonals, O(N) algebra instead of dense n^3."""

    def __init__(self, d11, d12, d21, d22):
        self.d = (d11, d12, d21, d22)

    @classmethod
    def identity_like(cls, t):
        one, zero = torch.ones_like(t), torch.zeros_like(t)
        return cls(one, zero, zero, one)

    def __add__(self, o):
        return BlockDiag2(*[a + b for a, b in zip(self.d, o.d)])

    def __sub__(self, o):
        return BlockDiag2(*[a - b for a, b in zip(self.d, o.d)])

    def __neg__(self):
        return BlockDiag2(*[-a for a in self.d])

    def scale(self, s):
        return BlockDiag2(*[s * a for a in self.d])

    def __matmul__(self, o):
        a, b, c, d = self.d
        e, f, g, h = o.d
        return BlockDiag2(a * e + b * g, a * f + b * h, c * e + d * g, c * f + d * h)

    def inv(self):
        a, b, c, d = self.d
        det = a * d - b * c
        return BlockDiag2(d / det, -b / det, -c / det, a / det)

    def dense(self):
        a, b, c, d = self.d
        top = torch.cat((torch.diag_embed(a), torch.diag_embed(b)), dim=2)
        bot = torch.cat((torch.diag_embed(c), torch.diag_embed(d)), dim=2)
        return torch.cat((top, bot), dim=1)

    def apply(self, X):
        """self @ X for a dense X [B, n, c] (n = 2N), in X's dtype: O(n c)."""
        N = X.shape[1] // 2
        a, b, c, d = [t.to(X.dtype)[:, :, None] for t in self.d]
        return torch.cat((a * X[:, :N] + b * X[:, N:], c * X[:, :N] + d * X[:, N:]), dim=1)

    def packed(self, dtype):
        """[4,B,N]: the four diagonals as the library takes a block-diagonal operator."""
        return torch.stack(self.d, dim=0).to(dtype).contiguous()


def _kz_branch(kz, negate=False):
    """The branch Im kz >= 0 of a square root: conj(kz) where Im kz < 0 for the kz of a homogeneous medium (rcwa.py:1145, 1218), -kz with
    `negate` for the square root of an eigenvalue (rcwa.py:1241)."""
    return torch.where(torch.imag(kz) < 0, -kz if negate else torch.conj(kz), kz)


def _halfspace_V(kx, ky, epsmu):
    """E->H map of a homogeneous half space, eps*mu = epsmu ([B] or scalar)        rcwa.py:1143-1147"""
    kz = _kz_branch(torch.sqrt(epsmu - kx ** 2 - ky ** 2))
    return BlockDiag2(-ky * kx / kz, -kz - ky ** 2 / kz, kz + kx ** 2 / kz, kx * ky / kz)


def _star_bd(Sm, Sn):
    """Star product of two block-diagonal S-matrices (rcwa.py:1287-1296), O(N)."""
    I = BlockDiag2.identity_like(Sm[0].d[0])
    t1 = (I - Sm[2] @ Sn[1]).inv()
    t2 = (I - Sn[1] @ Sm[2]).inv()
    return [Sn[0] @ t1 @ Sm[0], Sm[1] + Sm[3] @ t2 @ Sn[1] @ Sm[0], Sn[2] + Sn[0] @ t1 @ Sm[2] @ Sn[3], Sm[3] @ t2 @ Sn[3]]
