"""curope -- drop-in for CroCo's compiled RoPE2D extension (reference
``thirdparty/mast3r/dust3r/croco/models/curope``: ``kernels.cu`` behind ``curope.cpp``).

The reference's ``curope2d.py:6-9`` tries ``import curope`` first, so with this directory's parent
on ``PYTHONPATH`` (the entry that already provides ``mast3r_slam_backends``) the unchanged
``pos_embed.py`` picks the gfx950 kernel of ``csrc/rope.hip`` instead of its torch fallback.
"""
from mast3r_slam_backends import rope_2d

__all__ = ["rope_2d"]
