"""The eight symmetries of the square as augmentation codes (host only, numpy; DESIGN.md section 9, "Dihedral augmentation").

A code is three bits - 4: transpose, 2: reverse the rows, 1: reverse the columns - applied in that order (apply() is the
definition, cae_dihedral_rows of include/cae_hip.h the device's form of it).  "flips" are the codes 0 .. 3, which any plane
takes; "dihedral" adds the transposes and quarter turns 4 .. 7, which need a square plane.

codes(seed, epoch, n_case, group): the code of case j in epoch e is the draw of cae_bootstrap_sums' generator at position
(r = e, i = j) with n_unit = group: output x + 1 of splitmix64 seeded with `seed`, x = (e << 32) | j, the high 32 bits scaled
to the group.  A code belongs to the CASE, not to the row the shuffle gives it: the augmented epoch is the same under any
batch order and any number of ranks."""
import numpy as np

GROUPS = {"flips": 4, "dihedral": 8}


def check_group(name, what="augment"):
    """the size of the named group; an unknown name is a ValueError"""
    try:
        return GROUPS[name]
    except (KeyError, TypeError):
        raise ValueError(f"{what} must be one of {', '.join(GROUPS)}, got {name!r}") from None


def check_square(name, shapes, what="augment"):
    """`dihedral` transposes: every plane (.., h, w) of `shapes` must be square.  A ValueError names the first that is not."""
    if check_group(name, what) == 8:
        for shape in shapes:
            (h, w) = (int(shape[-2]), int(shape[-1]))
            if h != w:
                raise ValueError(f"{what}='dihedral' transposes, which needs square planes: got {h} x {w}; use 'flips'")


def check_seed(seed, what="augment_seed"):
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"{what} must be an integer from 0 to 2^64 - 1, got {seed!r}")
    return int(seed)


def inverse_code(code):
    """the code that undoes `code`: bit 2 is kept, bits 0 and 1 change places where it is set (5 <-> 6, the others themselves).
    An integer or an integer array."""
    code = np.asarray(code)
    swapped = (code & 4) | ((code & 1) << 1) | ((code & 2) >> 1)
    out = np.where((code & 4) != 0, swapped, code).astype(code.dtype if code.dtype.kind in "iu" else np.int32)
    return out if out.ndim else int(out)


def apply(a, code):
    """the numpy definition: `code` applied to the last two axes of a (a view, nothing is copied)"""
    code = int(code)
    if not 0 <= code < 8:
        raise ValueError(f"a code from 0 to 7 expected, got {code}")
    if code & 4:
        a = np.swapaxes(a, -1, -2)
    if code & 2:
        a = a[..., ::-1, :]
    if code & 1:
        a = a[..., ::-1]
    return a


def codes(seed, epoch, n_case, group):
    """the (n_case,) int32 codes of epoch `epoch`: bs_unit(seed, r = epoch, i = case, n_unit = group) of csrc/kernels_compare.h,
    in wrapping uint64 array arithmetic"""
    seed = check_seed(seed, "seed")
    (epoch, n_case, group) = (int(epoch), int(n_case), int(group))
    if group not in (4, 8):
        raise ValueError(f"group must be 4 or 8, got {group}")
    if not 0 <= epoch < 1 << 32 or not 0 <= n_case < 1 << 32:
        raise ValueError(f"epoch and n_case must lie within [0, 2^32), got {epoch} and {n_case}")
    u = lambda v: np.full(1, v, dtype=np.uint64)       # noqa: E731  (one-element arrays: array arithmetic wraps without a warning)
    x = np.arange(n_case, dtype=np.uint64) | (u(epoch) << u(32))
    z = u(seed) + (x + u(1)) * u(0x9E3779B97F4A7C15)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z = z ^ (z >> u(31))
    return (((z >> u(32)) * u(group)) >> u(32)).astype(np.int32)
