"""Warnings raised by pyxu_amd (mirrors the names of reference ``pyxu.info.warning`` that this package uses)."""

__all__ = ["DenseWarning"]


class DenseWarning(UserWarning):
    """A matrix-free algorithm reverted to a dense array (LinOp.svdvals with k >= min(shape) // 2)."""
