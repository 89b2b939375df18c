"""fractal-image-compression_amd -- MI355X (gfx950) grey encode hot path of bvk_ss19.

Import as `fic_amd` (see fic_amd.py at the repo root).  Everything that computes a block
match lives in csrc/ (HIP) behind the C ABI of include/fic.h; this package is the host-side
mirror of the reference's interface plus the multi-GPU plumbing.
"""
from . import capi, synth, sharding
from .capi import FicError, declared_symbols, geometry, write_run_gray, decode_gray_run, decode_rgb_run, encode_rgb, write_run_rgb
from .capi import encode_gray_quadtree, write_run_quadtree, decode_quadtree_run
from .capi import encode_rgb_quadtree, write_run_rgb_quadtree, decode_rgb_quadtree_run
from .capi import write_run_gray_iso, write_run_rgb_iso, decode_gray_iso_run, decode_rgb_iso_run
from .capi import encode_rgb_quadtree_iso, write_run_rgb_quadtree_iso, decode_rgb_quadtree_iso_run, debug_rgb_quadtree_iso_sse
from .capi import encode_gray_quadtree_budget, encode_rgb_quadtree_budget, encode_rgb_quadtree_iso_budget
from .capi import quadtree_leaves_for_bytes, debug_qt_select
from .capi import encode_gray_quadtree_rd, encode_rgb_quadtree_rd, encode_rgb_quadtree_iso_rd
from .capi import RgbEncoder
from .host import Encoder, QuadtreeEncoder, FractalCompression, RasterImage, encode_gray, encode_rgb_per_channel
from .sharding import ShardedEncoder, shard_spans, shard_planes, gather_records, pack_records, unpack_records

__all__ = ["capi", "synth", "sharding", "FicError", "declared_symbols", "geometry", "write_run_gray", "decode_gray_run", "decode_rgb_run", "encode_rgb", "write_run_rgb", "Encoder",
           "FractalCompression", "RasterImage", "encode_gray", "ShardedEncoder", "shard_spans", "shard_planes",
           "gather_records", "pack_records", "unpack_records", "encode_gray_quadtree", "write_run_quadtree",
           "decode_quadtree_run", "encode_rgb_quadtree", "write_run_rgb_quadtree", "decode_rgb_quadtree_run",
           "write_run_gray_iso", "write_run_rgb_iso", "decode_gray_iso_run", "decode_rgb_iso_run", "encode_rgb_quadtree_iso",
           "write_run_rgb_quadtree_iso", "decode_rgb_quadtree_iso_run", "debug_rgb_quadtree_iso_sse", "RgbEncoder",
           "encode_gray_quadtree_budget", "encode_rgb_quadtree_budget", "encode_rgb_quadtree_iso_budget", "quadtree_leaves_for_bytes",
           "debug_qt_select", "encode_gray_quadtree_rd", "encode_rgb_quadtree_rd", "encode_rgb_quadtree_iso_rd", "QuadtreeEncoder"]
