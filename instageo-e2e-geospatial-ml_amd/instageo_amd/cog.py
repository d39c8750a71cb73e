"""Cloud Optimized GeoTIFF output: overview pyramids built on the device and a tiled, overview-first file layout.

The reference's serving layer turns predictions into COGs with ``gdal_translate -of COG -co BLOCKSIZE=<chip_size> -co OVERVIEW_COUNT=6``
(``new_apps/backend/app/cog_converter.py``) and computes ``valid_pixels / class_counts / unique_values`` from the result.  GDAL is absent
here; this module is the stand-in, on top of :mod:`instageo_amd.tiff` and the kernels of ``cog.hip``.

The pyramid (stated in ``include/instageo_hip.h``).  Level 0 is the raster, H_0 x W_0; level k has H_k = ceil(H_{k-1} / 2) rows and
W_k = ceil(W_{k-1} / 2) columns.  Pixel (r, c) of level k has as children the pixels (2r..2r+1, 2c..2c+1) of level k-1 that lie inside
that level: 1, 2 or 4 of them.  Levels cascade: level k is computed from level k-1, never from level 0.

* ``mode``, for int8 class maps with a fill value: children equal to ``fill`` are ignored; if none is left the result is ``fill``;
  otherwise the value with the most children, ties to the smallest value.  The rule does not depend on child order, so it commutes with
  the eight D4 maps whenever H and W are multiples of 2^levels.  It makes no claim of equality with GDAL's ``MODE`` resampling.
* ``mean``, for float32 rasters with NaN as NODATA, band by band: the float32 sum of the children that are not NaN in row-major child
  order, divided by their count as float32 with IEEE round-to-nearest division; NaN if there are none.  Bit-reproducible and equal to
  numpy float32 arithmetic in the same order.

Device tensors go through ``ig_overview_mode`` / ``ig_overview_mean`` / ``ig_cog_tiles``; host arrays take a numpy path of the same
rules, so the writer works (and is tested) without a GPU.  Deflate runs on the host.

Not done: BigTIFF, LZW writing, predictor 3, GDAL's ghost-area metadata block, other resampling rules and argmax-of-mean class
overviews.  The mosaic of per-chip predictions into one canvas (the reference's ``gdal_merge`` step) is :mod:`instageo_amd.mosaic`.
"""
from __future__ import annotations

import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import tiff
from .prep import is_device
from .tiff import TiffError

BLOCKSIZES = (128, 256, 512)
MAX_LEVELS = 12  # of the entry points
MAX_CLASSES = 127  # of ig_overview_mode's histogram, and of an int8 class map
DEFLATE_THREADS = 8
_NAN_BITS = 0x7FC00000
_SUBFILE, _SUBFILE_REDUCED = 254, 1


def level_shapes(H: int, W: int, levels: Union[str, int] = "auto", blocksize: int = 256) -> List[Tuple[int, int]]:
    """[(H_k, W_k) for k = 1..n].  ``levels="auto"``: the fewest levels after which both sides are <= ``blocksize`` (at most 12); an int:
    that many, stopping early at 1 x 1."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"a raster has at least one row and one column (got {H} x {W})")
    levels = check_levels(levels)
    auto = levels == "auto"
    n = MAX_LEVELS if auto else levels
    out: List[Tuple[int, int]] = []
    while len(out) < n and ((max(H, W) > blocksize) if auto else (H, W) != (1, 1)):
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


def check_levels(levels: Union[str, int]) -> Union[str, int]:
    """'auto' or an int in 0..12 (a bool is neither); raises ValueError."""
    if isinstance(levels, str):
        if levels != "auto":
            raise ValueError(f"overview_levels must be 'auto' or an int in 0..{MAX_LEVELS} (got {levels!r})")
        return levels
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= int(levels) <= MAX_LEVELS:
        raise ValueError(f"overview_levels must be 'auto' or an int in 0..{MAX_LEVELS} (got {levels!r})")
    return int(levels)


def check_cog_options(cog: bool, blocksize: int = 256, levels: Union[str, int] = "auto", compress: Optional[str] = "deflate",
                      chip_mode: bool = False, ncls: Optional[int] = None) -> None:
    """The ``test.cog*`` / ``test.overview_levels`` keys, checked before any work (chip / tile inference, run.py).  ``ncls``: the model's
    classes when known; with ``cog`` more than 127 are refused (the class histogram of ``ig_overview_mode`` has 127 + 1 slots)."""
    if isinstance(blocksize, bool) or blocksize not in BLOCKSIZES:
        raise ValueError(f"cog_blocksize must be one of {BLOCKSIZES} (got {blocksize!r})")
    check_levels(levels)
    if compress not in (None, "none", "deflate"):
        raise ValueError(f"cog_compress must be 'deflate' or 'none' (got {compress!r})")
    if cog and ncls is not None and ncls > MAX_CLASSES:
        raise ValueError(f"test.cog handles class maps of at most {MAX_CLASSES} classes (the model has {ncls})")
    if cog and chip_mode:
        raise ValueError("test.cog needs mode=tile_inference: per-chip COGs are not produced (a chip is one block); convert single files "
                         "with instageo_amd.cog.convert")


# ---- the two rules on host arrays ------------------------------------------------------------------------------------------------------
def _children(a: np.ndarray, pad) -> Tuple[np.ndarray, ...]:
    """The four child planes of the next level of ``a`` (..., H, W), missing children = ``pad``."""
    H, W = a.shape[-2:]
    if H % 2 or W % 2:
        a = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(0, H % 2), (0, W % 2)], constant_values=pad)
    return a[..., 0::2, 0::2], a[..., 0::2, 1::2], a[..., 1::2, 0::2], a[..., 1::2, 1::2]


def _mode_level(a: np.ndarray, fill: int) -> np.ndarray:
    v = [c.astype(np.int16) for c in _children(a, fill)]
    best = np.full(v[0].shape, fill, dtype=np.int16)
    bestn = np.zeros(v[0].shape, dtype=np.int16)
    for i in range(4):
        n = sum((v[j] == v[i]).astype(np.int16) for j in range(4))
        better = (v[i] != fill) & ((n > bestn) | ((n == bestn) & (v[i] < best)))
        best = np.where(better, v[i], best)
        bestn = np.where(better, n, bestn)
    return best.astype(np.int8)


def _mean_level(a: np.ndarray) -> np.ndarray:
    v = _children(a, np.float32(np.nan))
    s = np.zeros(v[0].shape, dtype=np.float32)
    n = np.zeros(v[0].shape, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c in v:
            ok = ~np.isnan(c)
            s = np.where(ok, np.where(n > 0, s + c, c), s).astype(np.float32)
            n = n + ok.astype(np.float32)
        out = (s / n).astype(np.float32)
    out[n == 0] = np.uint32(_NAN_BITS).view(np.float32)
    return out


def class_histogram(classmap: np.ndarray, ncls: int, fill: int = -1) -> np.ndarray:
    """(ncls + 1,) int64: the pixels of every class in [0, ncls) that is not ``fill``; the last slot counts ``fill`` and every other value
    (what ``ig_overview_mode`` accumulates into ``counts``)."""
    v = np.asarray(classmap).astype(np.int64).ravel()
    idx = np.where((v != fill) & (v >= 0) & (v < ncls), v, ncls)
    return np.bincount(idx, minlength=int(ncls) + 1).astype(np.int64)


def build_overviews(raster, kind: str = "mode", levels: Union[str, int] = "auto", fill: int = -1, blocksize: int = 256,
                    ncls: Optional[int] = None, counts=None) -> list:
    """-> [level 0 (``raster`` itself), level 1, ...], ready for :func:`write_cog`.  ``raster``: (H, W) or (bands, H, W); a HIP tensor goes
    through the kernels and gives device tensors, anything else takes the numpy path and gives arrays.  ``kind="mode"`` needs int8 (one
    band on the device), ``"mean"`` float32.  ``levels`` / ``blocksize``: :func:`level_shapes`.  ``counts`` ((ncls + 1,) int64 of the
    raster's kind, mode only) += the class histogram of ``raster`` (:func:`class_histogram`; on the device it comes out of the pyramid
    kernel, which then builds one level even when none is asked for)."""
    if kind not in ("mode", "mean"):
        raise ValueError(f"kind must be 'mode' or 'mean' (got {kind!r})")
    if counts is not None and (kind != "mode" or ncls is None):
        raise ValueError("counts needs kind='mode' and ncls")
    dev = is_device(raster)
    if not dev:
        raster = np.asarray(raster.cpu() if hasattr(raster, "cpu") else raster)
    want = "int8" if kind == "mode" else "float32"
    if str(raster.dtype).replace("torch.", "") != want:
        raise ValueError(f"kind={kind!r} needs a {want} raster (got {raster.dtype})")
    if raster.ndim not in (2, 3):
        raise ValueError("a raster is (H, W) or (bands, H, W)")
    H, W = raster.shape[-2:]
    n = len(level_shapes(H, W, levels, blocksize))
    out = [raster]
    if not dev:
        if counts is not None:
            counts += class_histogram(raster, ncls, fill)
        for _ in range(n):
            out.append(_mode_level(out[-1], int(fill)) if kind == "mode" else _mean_level(out[-1]))
        return out
    from . import ops

    if kind == "mode":
        if raster.ndim == 3 and raster.shape[0] != 1:
            raise ValueError("on the device a class map has one band")
        if n == 0 and counts is None:
            return out
        lv = ops.overview_mode(raster.reshape(H, W), max(n, 1), int(fill), int(ncls) if ncls is not None else 1, counts)[:n]
        return out + [l.view(1, *l.shape) if raster.ndim == 3 else l for l in lv]
    if n == 0:
        return out
    lv = ops.overview_mean(raster.reshape(-1, H, W), n)
    return out + [l if raster.ndim == 3 else l[0] for l in lv]


def seg_stats(counts) -> Dict[str, Any]:
    """The reference's segmentation statistics (``compute_seg_stats``) from a class histogram (ncls + 1,) whose last slot holds the
    invalid pixels: {"valid_pixels", "class_counts": {str(class): pixels, only > 0}, "unique_values"}."""
    c = [int(x) for x in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    cc = {str(i): n for i, n in enumerate(c[:-1]) if n > 0}
    return {"valid_pixels": sum(c[:-1]), "class_counts": cc, "unique_values": len(cc)}


# ---- the writer --------------------------------------------------------------------------------------------------------------------------
def _pad_bits(dtype: np.dtype, nodata) -> int:
    """The bit pattern (as an unsigned int) of the value outside the raster in the edge tiles: NODATA, else NaN for floats and 0."""
    if dtype.kind == "f":
        v = np.float32(np.nan) if nodata is None else np.float32(nodata)
        return _NAN_BITS if np.isnan(v) else int(v.view(np.uint32))
    v = 0 if nodata is None or float(nodata) != int(nodata) else int(nodata)
    info = np.iinfo(dtype)
    v = v if info.min <= v <= info.max else 0
    return int(np.array(v, dtype=dtype).view(f"u{dtype.itemsize}"))


def _tiles_host(a: np.ndarray, tile: int, pad_bits: int, predictor: int) -> np.ndarray:
    """numpy twin of ``ig_cog_tiles``: (bands, H, W) -> (bands, ny, nx, tile, tile), as the unsigned view of the elements."""
    u = np.ascontiguousarray(a).view(f"<u{a.dtype.itemsize}")
    B, H, W = u.shape
    ny, nx = -(-H // tile), -(-W // tile)
    full = np.full((B, ny * tile, nx * tile), pad_bits, dtype=u.dtype)
    full[:, :H, :W] = u
    t = full.reshape(B, ny, tile, nx, tile).transpose(0, 1, 3, 2, 4)
    if predictor == 2:
        d = t.copy()
        d[..., 1:] = t[..., 1:] - t[..., :-1]  # unsigned: wraps in the element's width
        t = d
    return np.ascontiguousarray(t)


def _tile_bytes(level, tile: int, pad_bits: int, predictor: int) -> Tuple[List[bytes], int, int, int, np.dtype]:
    """-> (the raw bytes of the tiles in (band, ty, tx) order, bands, H, W, the little-endian dtype)."""
    if is_device(level):
        from . import ops

        t = level if level.dim() == 3 else level.unsqueeze(0)
        if t.dim() != 3:
            raise TiffError("a level must be (H, W) or (bands, H, W)")
        dt = np.dtype(str(t.dtype).replace("torch.", ""))
        tiles = ops.cog_tiles(t.contiguous(), tile, pad_bits, predictor).cpu().numpy()
        B, H, W = t.shape
    else:
        a = np.asarray(level)
        a = a[None] if a.ndim == 2 else a
        if a.ndim != 3:
            raise TiffError("a level must be (H, W) or (bands, H, W)")
        if a.dtype == np.bool_:
            a = a.astype(np.uint8)
        dt = a.dtype
        if dt.kind not in "uif" or dt.itemsize not in (1, 2, 4):
            raise TiffError(f"unsupported dtype {dt}")
        tiles = _tiles_host(a.astype(dt.newbyteorder("<"), copy=False), tile, pad_bits, predictor)
        B, H, W = a.shape
    if dt.kind not in "uif" or dt.itemsize not in (1, 2, 4) or (dt.kind == "f" and dt.itemsize != 4):
        raise TiffError(f"unsupported dtype {dt}")
    flat = tiles.reshape(-1, tile * tile)
    return [flat[i].tobytes() for i in range(flat.shape[0])], B, H, W, dt.newbyteorder("<")


def write_cog(path: str, levels: Sequence, profile: Optional[Dict[str, Any]] = None, blocksize: int = 256,
              compress: Optional[str] = "deflate", predictor: Optional[int] = None) -> str:
    """Write ``levels`` ([level 0, level 1, ...] of :func:`build_overviews`: device tensors or arrays, (H, W) or (bands, H, W), one dtype)
    as a classic little-endian tiled TIFF in the COG layout: header | IFD 0 (full resolution, the georeferencing tags of
    ``profile["tags"]`` copied verbatim as :func:`tiff.write` does) | the overview IFDs in decreasing size (NewSubfileType = 1, no
    georeferencing) | all out-of-line tag values | the tile data from the smallest overview to level 0, TileOffsets ascending inside each
    level.  GDAL_NODATA stands on every IFD.  Several bands: PlanarConfiguration 2.  Tiles are ``blocksize`` x ``blocksize``; the part of
    an edge tile outside the raster holds NODATA (NaN for floats without one, else 0).  ``compress``: "deflate" (zlib level 6, in a pool of
    at most 8 threads) | None; ``predictor``: None | 1 | 2 (horizontal differencing, integers only).  Beyond 4 GiB: ``TiffError``."""
    if isinstance(blocksize, bool) or int(blocksize) < 16 or int(blocksize) % 16:
        raise TiffError(f"blocksize must be a multiple of 16 (got {blocksize!r})")
    tile = int(blocksize)
    if compress not in (None, "none", "deflate"):
        raise TiffError(f"unsupported compression {compress!r}")
    deflate = compress == "deflate"
    pred = 1 if predictor is None else int(predictor)
    if pred not in (1, 2):
        raise TiffError(f"unsupported predictor {predictor!r} (1 or 2)")
    if len(levels) == 0:
        raise TiffError("write_cog needs at least level 0")
    first = levels[0]
    dt0 = np.dtype(str(first.dtype).replace("torch.", "")) if is_device(first) else np.asarray(first).dtype
    if pred == 2 and dt0.kind == "f":
        raise TiffError("predictor 2 is for integer samples")
    tags = dict((profile or {}).get("tags", {}))
    nd = (profile or {}).get("nodata")
    if nd is not None and 42113 not in tags:
        tags[42113] = (2, repr(float(nd)) if float(nd) != int(nd) else str(int(nd)))
    if nd is None and 42113 in tags:
        try:
            nd = float(tags[42113][1])
        except (TypeError, ValueError):
            nd = None
    pad_bits = _pad_bits(np.dtype("uint8") if dt0 == np.bool_ else dt0, nd)

    metas = []  # per level: (tile payloads, bands, H, W, dtype)
    for k, lv in enumerate(levels):
        raw, B, H, W, dt = _tile_bytes(lv, tile, pad_bits, pred)
        if k and (B, dt) != (metas[0][1], metas[0][4]):
            raise TiffError(f"level {k} has {B} band(s) of {dt}, level 0 has {metas[0][1]} of {metas[0][4]}")
        if k and (H, W) != ((metas[-1][2] + 1) // 2, (metas[-1][3] + 1) // 2):
            raise TiffError(f"level {k} is {H} x {W}; after {metas[-1][2]} x {metas[-1][3]} comes {(metas[-1][2] + 1) // 2} x {(metas[-1][3] + 1) // 2}")
        metas.append((raw, B, H, W, dt))
    if deflate:
        everything = [t for m in metas for t in m[0]]
        with ThreadPoolExecutor(max_workers=max(1, min(DEFLATE_THREADS, len(everything)))) as pool:  # zlib releases the GIL
            packed = list(pool.map(lambda b: zlib.compress(b, 6), everything))
        o = 0
        for i, m in enumerate(metas):
            metas[i] = (packed[o : o + len(m[0])],) + m[1:]
            o += len(m[0])

    T = tiff
    ifds: List[List[Tuple[int, int, int, bytes]]] = []
    for k, (data, B, H, W, dt) in enumerate(metas):
        e = [T._entry(T._W, 4, (W,)), T._entry(T._H, 4, (H,)), T._entry(T._BPS, 3, (dt.itemsize * 8,) * B),
             T._entry(T._COMP, 3, (8 if deflate else 1,)), T._entry(T._PHOTO, 3, (1,)), T._entry(T._SPP, 3, (B,)),
             T._entry(T._PLANAR, 3, (2 if B > 1 else 1,)), T._entry(T._TILE_W, 4, (tile,)), T._entry(T._TILE_H, 4, (tile,)),
             T._entry(T._TILE_OFF, 4, (0,) * len(data)), T._entry(T._TILE_CNT, 4, tuple(len(d) for d in data)),
             T._entry(T._FMT, 3, (T._FMT_OF[dt.kind],) * B)]  # fmt: skip
        if k:
            e.append(T._entry(_SUBFILE, 4, (_SUBFILE_REDUCED,)))
        if pred == 2:
            e.append(T._entry(T._PRED, 3, (2,)))
        if B > 1:
            e.append(T._entry(T._EXTRA, 3, (0,) * (B - 1)))
        for tag, (typ, values) in tags.items():
            if k == 0 or int(tag) == 42113:
                e.append(T._entry(int(tag), int(typ), values))
        e.sort(key=lambda x: x[0])
        ifds.append(e)
    # layout: header | IFDs | out-of-line values | tiles, smallest level first
    pos = 8
    ifd_at = []
    for e in ifds:
        ifd_at.append(pos)
        pos += 2 + 12 * len(e) + 4
    value_at: List[Dict[int, int]] = []
    for e in ifds:
        at = {}
        for tag, typ, cnt, payload in e:
            if len(payload) > 4:
                at[tag] = pos
                pos += len(payload) + (len(payload) & 1)
        value_at.append(at)
    offsets: List[List[int]] = [[] for _ in metas]
    for k in range(len(metas) - 1, -1, -1):
        for d in metas[k][0]:
            offsets[k].append(pos)
            pos += len(d) + (len(d) & 1)
    if pos >= (1 << 32):
        raise TiffError("raster too large for classic TIFF")
    with open(path, "wb") as f:
        f.write(struct.pack("<2sHI", b"II", 42, ifd_at[0]))
        for k, e in enumerate(ifds):
            f.write(struct.pack("<H", len(e)))
            for tag, typ, cnt, payload in e:
                if tag == T._TILE_OFF:
                    payload = struct.pack(f"<{cnt}I", *offsets[k])
                if len(payload) <= 4:
                    f.write(struct.pack("<HHI4s", tag, typ, cnt, payload.ljust(4, b"\x00")))
                else:
                    f.write(struct.pack("<HHII", tag, typ, cnt, value_at[k][tag]))
            f.write(struct.pack("<I", ifd_at[k + 1] if k + 1 < len(ifds) else 0))
        for k, e in enumerate(ifds):
            for tag, typ, cnt, payload in e:
                if len(payload) > 4:
                    if tag == T._TILE_OFF:
                        payload = struct.pack(f"<{cnt}I", *offsets[k])
                    f.write(payload + b"\x00" * (len(payload) & 1))
        for k in range(len(metas) - 1, -1, -1):
            for d in metas[k][0]:
                f.write(d)
                if len(d) & 1:
                    f.write(b"\x00")
    return path


# ---- the checker -------------------------------------------------------------------------------------------------------------------------
def validate_cog(path: str) -> List[str]:
    """The violations of the COG layout in ``path`` ([] = a valid COG as far as this checks): every IFD tiled with block sides that are
    multiples of 16; every IFD before any tile data; the overviews follow the ceil(/2) chain and shrink strictly; NewSubfileType marks
    the overviews and only them; TileOffsets ascend inside each level and a smaller level's data lies before a larger one's."""
    with open(path, "rb") as f:
        buf = f.read()
    try:
        h = tiff._Header(path, buf)
        chain = tiff._ifd_chain(buf, h.bo, h.first_ifd)
        ifds = [tiff._read_ifd(buf, h.bo, off) for off in chain]
    except (struct.error, IndexError) as e:
        raise TiffError(f"{path}: truncated or corrupt TIFF ({e})") from e
    bad: List[str] = []
    one = lambda t, tag, d=None: t[tag][1][0] if tag in t else d  # noqa: E731
    spans = []  # per IFD: (first tile offset, end of the last tile) or None
    ifd_end = 0
    for k, (off, t) in enumerate(zip(chain, ifds)):
        n = struct.unpack_from(h.bo + "H", buf, off)[0]
        ifd_end = max(ifd_end, off + 2 + 12 * n + 4)
        if tiff._TILE_OFF not in t:
            bad.append(f"IFD {k}: not tiled (strips)")
            spans.append(None)
            continue
        tw, th = one(t, tiff._TILE_W, 0), one(t, tiff._TILE_H, 0)
        if tw <= 0 or th <= 0 or tw % 16 or th % 16:
            bad.append(f"IFD {k}: block size {tw} x {th} is no multiple of 16")
        offs, cnts = t[tiff._TILE_OFF][1], t[tiff._TILE_CNT][1]
        if any(b <= a for a, b in zip(offs, offs[1:])):
            bad.append(f"IFD {k}: TileOffsets do not ascend")
        spans.append((min(offs), max(o + c for o, c in zip(offs, cnts))))
        sub = one(t, _SUBFILE, 0)
        if k == 0 and sub & _SUBFILE_REDUCED:
            bad.append("IFD 0: NewSubfileType marks the full-resolution image as reduced")
        if k > 0 and not sub & _SUBFILE_REDUCED:
            bad.append(f"IFD {k}: an overview without NewSubfileType = 1")
        if k > 0:
            pw, ph = one(ifds[k - 1], tiff._W), one(ifds[k - 1], tiff._H)
            w, hh = one(t, tiff._W), one(t, tiff._H)
            if (hh, w) != ((ph + 1) // 2, (pw + 1) // 2) or hh * w >= ph * pw:
                bad.append(f"IFD {k}: {hh} x {w} does not follow {ph} x {pw} (want {(ph + 1) // 2} x {(pw + 1) // 2}, strictly smaller)")
    starts = [s[0] for s in spans if s]
    if starts and min(starts) < ifd_end:
        bad.append(f"tile data at {min(starts)} before the end of the IFDs at {ifd_end}")
    for k in range(1, len(spans)):
        if spans[k] and spans[k - 1] and spans[k][1] > spans[k - 1][0]:
            bad.append(f"IFD {k}: its data (to {spans[k][1]}) does not lie before that of IFD {k - 1} (from {spans[k - 1][0]})")
    return bad


def convert(src_path: str, dst_path: str, kind: Optional[str] = None, levels: Union[str, int] = "auto", blocksize: int = 256,
            compress: Optional[str] = "deflate", predictor: Optional[int] = None, fill: Optional[int] = None,
            device: Optional[str] = None) -> str:
    """Any TIFF :func:`tiff.read` can read -> a COG.  Unless ``kind`` is given, int8 becomes ``mode`` and float32 ``mean`` (other sample
    types have no rule here).  ``fill`` (mode): the file's NODATA when it has one, else -1.  ``device`` (e.g. "cuda") builds the pyramid
    with the kernels; None uses the numpy path."""
    arr, profile = tiff.read(src_path)
    if kind is None:
        kind = {"int8": "mode", "float32": "mean"}.get(arr.dtype.name)
        if kind is None:
            raise ValueError(f"{src_path}: no overview rule for {arr.dtype.name} samples (int8 -> mode, float32 -> mean)")
    if fill is None:
        nd = profile.get("nodata")
        fill = int(nd) if nd is not None and -128 <= nd <= 127 and float(nd) == int(nd) else -1
    if device is None:
        lv = build_overviews(arr, kind, levels, fill, blocksize)
    else:
        import torch

        t = torch.from_numpy(arr).to(device)
        if kind == "mode":  # band by band: the kernel takes one class map
            per = [build_overviews(t[b], kind, levels, fill, blocksize) for b in range(t.shape[0])]
            lv = [torch.stack([p[k] for p in per]) for k in range(len(per[0]))]
        else:
            lv = build_overviews(t, kind, levels, fill, blocksize)
    return write_cog(dst_path, lv, profile, blocksize, compress, predictor)
