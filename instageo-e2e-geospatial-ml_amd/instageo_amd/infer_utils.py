"""Chip / sliding-window inference (reference: ``instageo/model/infer_utils.py:37-136``).

The loop ``model(data) -> argmax(dim=1) -> int8`` (infer_utils.py:93-101) runs entirely on the device (``ig_argmax_i8``); the
per-chip rasters are written as ``prediction_*.tif`` with the source chip's georeferencing tags by the same 4-thread pool
structure (``save_prediction``, infer_utils.py:37-54, through :mod:`instageo_amd.tiff` instead of rasterio).

``sliding_window_inference`` is BASELINE.json configs[3]: a 10980^2 tile -> 49 x 49 windows of 224 (the window rule of
``process_test``, dataloader.py:655-664), gathered + normalised by ONE kernel launch per batch (``ig_normalize_windows``),
windows partitioned contiguously over ranks, final gather; ``stitch_windows`` puts the class maps back on the tile canvas
(overlapping windows: every pixel takes the window whose centre is nearest), ``tile_inference`` does file -> file.

``blended_window_inference`` is the second tile path (``tile_inference(blend="mean" | "gaussian")``): any H x W tile, optionally a
last window row / column at the edge (``cover_edges``), per-window class probabilities averaged on the canvas with a separable
window weight (``ig_window_blend_accumulate``: gather form, no atomics, bit-identical for any batch size), then one
``ig_window_blend_finalize`` -> class map + optional probability raster.  ``tta="flips" | "d4"`` runs every window under the flips /
all eight transforms of the square (``ig_d4_apply`` before and after the forward pass) and averages them on the same canvas
(``ig_window_blend_accumulate_tta``); ``uncertainty`` adds the entropy / top-two-margin raster (``ig_window_blend_uncertainty``).
"""
from __future__ import annotations

import json
import os
from concurrent.futures import Executor, ThreadPoolExecutor
from dataclasses import dataclass
from functools import partial
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import distributed as D
from . import cog as cogmod
from . import ops, postprocess, tiff, vectorize, zonal
from .calibration import check_temperature
from .dataloader import d4_codes, d4_inverse, gather_windows, origins_tensor, window_grid, window_origins


@dataclass(frozen=True)
class OutputOptions:
    """What inference writes of a finished class map besides the map: the output keywords of :func:`tile_inference`, with its defaults
    (:func:`chip_inference` has the first seven)."""
    min_region: int = 0
    connectivity: int = 4
    sieve_passes: int = 8
    save_regions: bool = False
    save_polygons: bool = False
    zones: Optional[str] = None
    zone_id_property: Optional[str] = None
    cog: bool = False
    cog_blocksize: int = 256
    overview_levels: Union[str, int] = "auto"
    cog_compress: Optional[str] = "deflate"

    def check(self, model, chip_mode: bool = False) -> None:
        """ValueError for options that cannot work, the first of the four checks that objects: before any file or device is touched.
        ``model``: only its configured ``num_classes`` is read; None (nothing to ask) leaves the checks that need it out."""
        ncls = getattr(getattr(getattr(model, "net", model), "cfg", None), "num_classes", None)
        postprocess.check_region_options(self.min_region, self.connectivity, self.sieve_passes, self.save_regions, ncls == 1)
        vectorize.check_polygon_options(self.save_polygons, ncls == 1)
        zonal.check_zone_options(self.zones, ncls == 1)
        cogmod.check_cog_options(self.cog, self.cog_blocksize, self.overview_levels, self.cog_compress, chip_mode=chip_mode, ncls=ncls)


def save_prediction(prediction: np.ndarray, file_name: str, output_folder: str, profile: Optional[Dict[str, Any]] = None,
                    kind: str = "prediction") -> str:
    """Save one prediction as a TIFF next to the reference's naming (``chip`` -> ``prediction`` in the base name,
    infer_utils.py:51-54); ``profile`` = the source chip's profile (georeferencing tags are copied, count = 1).  ``kind`` replaces
    "prediction" in the name (``probability`` and ``uncertainty`` rasters of the blended tile path)."""
    path = _output_path(file_name, output_folder, kind)
    tiff.write(path, prediction, profile)
    return path


def _output_path(file_name: str, output_folder: str, kind: str, ext: Optional[str] = None) -> str:
    """``save_prediction``'s naming; ``ext`` replaces the extension (``regions_*.csv``, ``polygons_*.geojson``, ``zones_*.csv``)."""
    base = os.path.basename(str(file_name))
    out = base.replace("chip", kind) if "chip" in base else f"{kind}_" + base
    if ext is not None:
        out = os.path.splitext(out)[0] + ext
    elif not out.lower().endswith((".tif", ".tiff")):
        out = os.path.splitext(out)[0] + ".tif"
    return os.path.join(output_folder, out)


def save_cog(raster: torch.Tensor, kind: str, file_name: str, output_folder: str, profile: Optional[Dict[str, Any]], opts: OutputOptions,
             name_kind: str = "prediction", fill: int = -1, ncls: Optional[int] = None) -> str:
    """Write one raster still on the device as a Cloud Optimized GeoTIFF under :func:`save_prediction`'s name: the overviews by
    ``kind`` ("mode" for the int8 class map, "mean" for float32 rasters) come from the device (:func:`cog.build_overviews`), level 0 holds
    the pixels :func:`save_prediction` would write.  ``ncls``: also write ``cogstats_*.json``, the reference's segmentation statistics
    (:func:`cog.seg_stats`) from the class histogram the pyramid kernel takes along; more classes than its 127 slots: the raster is
    written without the statistics."""
    path = _output_path(file_name, output_folder, name_kind)
    if ncls is not None and ncls > cogmod.MAX_CLASSES:
        ncls = None
    counts = torch.zeros(ncls + 1, dtype=torch.int64, device=raster.device) if ncls is not None else None
    levels = cogmod.build_overviews(raster, kind, opts.overview_levels, fill, opts.cog_blocksize, ncls=ncls, counts=counts)
    cogmod.write_cog(path, levels, profile, opts.cog_blocksize, opts.cog_compress)
    if counts is not None:
        with open(_output_path(file_name, output_folder, "cogstats", ".json"), "w") as f:
            json.dump(cogmod.seg_stats(counts.cpu().numpy()), f, sort_keys=True)
    return path


def _engine_of(model):
    net = getattr(model, "net", model)
    return net, net.engine


def _profile_of(file_name: str, dtype: np.dtype) -> Optional[Dict[str, Any]]:
    """infer_utils.py:103-113: the source profile with count=1 and the prediction dtype; None for in-memory chips."""
    if not (isinstance(file_name, str) and os.path.isfile(file_name) and file_name.lower().endswith((".tif", ".tiff"))):
        return None
    prof = dict(tiff.read_profile(file_name))
    prof.update(count=1, dtype=np.dtype(dtype).name)
    if np.dtype(dtype) == np.int8:
        prof["nodata"] = None  # the chip's NODATA value (-9999) does not exist in an int8 class map
        prof["tags"] = {k: v for k, v in prof["tags"].items() if k != 42113}
    return prof


@torch.no_grad()
def chip_inference(dataloader, output_folder: str, model, device: str = "gpu", num_workers: int = 4, min_region: int = 0,
                   connectivity: int = 4, sieve_passes: int = 8, save_regions: bool = False, zones: Optional[str] = None,
                   zone_id_property: Optional[str] = None, save_polygons: bool = False) -> Dict:
    """Run inference on chips and save one int8 class map (float32 for single-channel regression heads) per chip as
    ``prediction_*.tif``.  Returns {} (the reference returns CodeCarbon numbers; there is no tracker here).

    ``min_region``, ``connectivity``, ``sieve_passes``, ``save_regions``, ``save_polygons``, ``zones`` and ``zone_id_property`` are those
    of :func:`tile_inference`, per chip (``zones`` in the chips' coordinate system).  With the defaults none of them runs."""
    opts = OutputOptions(min_region=min_region, connectivity=connectivity, sieve_passes=sieve_passes, save_regions=save_regions,
                         save_polygons=save_polygons, zones=zones, zone_id_property=zone_id_property)
    opts.check(model, chip_mode=True)
    zone_list = zonal.read_zones(zones, zone_id_property) if zones is not None else None
    os.makedirs(output_folder, exist_ok=True)
    net, eng = _engine_of(model)
    net.eval()
    with ThreadPoolExecutor(max_workers=num_workers) as executor:
        for (data, _), file_names in dataloader:
            data = data.to("cuda" if device == "gpu" else device)
            logits = eng.forward(data, training=False, save=False)
            regression = logits.shape[1] == 1  # a single output channel
            profiles = [_profile_of(f, np.float32 if regression else np.int8) for f in file_names]
            if regression:
                pred = logits.squeeze(1)
            else:
                pred = _write_products(ops.argmax_i8(logits), list(zip(file_names, profiles)), output_folder, fill=-1, ncls=logits.shape[1],
                                       opts=opts, zone_list=zone_list, executor=executor)
            for fut in [executor.submit(save_prediction, p, f, output_folder, prof) for p, f, prof in zip(pred.cpu().numpy(), file_names, profiles)]:
                fut.result()
    return {}


def _write_products(maps: torch.Tensor, targets: Sequence[Tuple[str, Optional[Dict[str, Any]]]], output_folder: str, fill: int, ncls: int,
                    opts: OutputOptions, zone_list=None, executor: Optional[Executor] = None) -> torch.Tensor:
    """Everything ``opts`` asks of finished class maps but the rasters: ``maps`` (n, H, W) int8 on the device, ``targets`` the n (file name,
    profile) pairs the products are named and georeferenced after -> the maps to write.  In this order: the sieve (``min_region`` > 0);
    ONE labelling of the sieved maps, shared by the region table and the rings, so both describe the same regions; ``regions_*.csv`` and
    ``polygons_*.geojson`` per image, through ``executor`` when there is one (waited for before returning); ``zones_*.csv`` per image with
    that image's profile, tallied on the device meanwhile (``zone_list``: :func:`zonal.read_zones`, ``ncls`` classes).  With the defaults
    nothing is launched and ``maps`` comes back untouched."""
    if opts.min_region > 0:
        maps, _ = postprocess.sieve_class_map(maps, opts.min_region, opts.connectivity, fill, opts.sieve_passes)
    jobs = []
    if opts.save_regions or opts.save_polygons:
        labels = postprocess.label_regions(maps, opts.connectivity, fill)
        table = postprocess.region_table(maps, opts.connectivity, fill, labels=labels)
        rings = vectorize.region_rings(maps, opts.connectivity, fill, labels=labels) if opts.save_polygons else None
        for i, (name, prof) in enumerate(targets):
            rows = postprocess.table_of_image(table, i)
            if opts.save_regions:
                jobs.append((postprocess.write_region_csv, (_output_path(name, output_folder, "regions", ".csv"), rows, prof)))
            if opts.save_polygons:
                jobs.append((vectorize.write_geojson, (_output_path(name, output_folder, "polygons", ".geojson"),
                                                       *vectorize.rings_of_image(*rings, i), rows, prof)))
    pending = [executor.submit(fn, *args) if executor is not None else fn(*args) for fn, args in jobs]
    if zone_list is not None:
        for m, (name, prof) in zip(maps, targets):
            ids, counts = zonal.zone_table(m, zone_list, ncls, fill, prof)
            zonal.write_zone_csv(_output_path(name, output_folder, "zones", ".csv"), ids, counts, prof)
    if executor is not None:
        for fut in pending:
            fut.result()
    return maps


def _write_raster(raster: torch.Tensor, name_kind: str, overview_kind: str, profile: Dict[str, Any], file_name: str, output_folder: str,
                  opts: OutputOptions, classes: Optional[Tuple[int, int]] = None) -> str:
    """One raster still on the device -> ``<name_kind>_*.tif`` (prediction | probability | uncertainty): a strip file, or with ``opts.cog`` a
    Cloud Optimized GeoTIFF with ``overview_kind`` (mode | mean) overviews.  ``classes`` = (fill, ncls) marks the class map: its mode
    ignores ``fill``, and only it gets ``cogstats_*.json``."""
    if not opts.cog:
        return save_prediction(raster.cpu().numpy(), file_name, output_folder, profile, kind=name_kind)
    fill, ncls = classes if classes is not None else (-1, None)
    return save_cog(raster, overview_kind, file_name, output_folder, profile=profile, opts=opts, name_kind=name_kind, fill=fill, ncls=ncls)


@torch.no_grad()
def sliding_window_inference(tile: torch.Tensor, model, mean: Sequence[float], std: Sequence[float], temporal_size: int = 1,
                             crop_size: int = 224, stride: int = 224, batch_size: int = 64,
                             constant_multiplier: Optional[float] = None, gather: bool = True
                             ) -> Tuple[Optional[torch.Tensor], List[Tuple[int, int]]]:
    """tile (T*C, S, S) int16|f32 on the device -> int8 class maps (n_windows, crop, crop) on rank 0.

    Every rank takes a contiguous block of the window list (no data-path collective); per batch ONE ``ig_normalize_windows``
    launch gathers and normalises its windows straight from the tile, then the forward pass and the fused argmax;
    ``gather`` collects the maps on rank 0 over RCCL.  Returns (maps or None on non-zero ranks, all window origins).
    """
    net, eng = _engine_of(model)
    net.eval()
    S = tile.shape[-1]
    origins = window_origins(S, crop_size, stride)
    world = D.world_size()
    rank = torch.distributed.get_rank() if world > 1 else 0
    lo, hi = D.shard_range(len(origins), rank, world)
    mine = origins_tensor(origins[lo:hi], tile.device)
    n = hi - lo
    out = torch.empty((n, crop_size, crop_size), dtype=torch.int8, device=tile.device)
    C = tile.shape[0] // temporal_size
    # balanced batches: ceil(n / batch_size) batches of nearly equal size (2401 windows at 108 per batch = 23 x 104-105, not 22 x 108 + 25:
    # a small ragged batch runs the persistent GEMM grids mostly empty and allocates a workspace of its own)
    nbatch = max(1, -(-n // batch_size))
    bs = -(-n // nbatch) if n else 1
    xbuf = torch.empty((max(bs, 1), C, temporal_size, crop_size, crop_size), dtype=torch.float32, device=tile.device)
    for i in range(0, n, bs):
        k = min(bs, n - i)
        x, _ = gather_windows(tile, mine[i : i + k], mean, std, temporal_size, crop_size, constant_multiplier, out=xbuf[:k])
        logits = eng.forward(x, training=False, save=False)
        ops.argmax_i8(logits, out[i : i + k])
    if gather and D.dp_active():
        counts = [D.shard_range(len(origins), r, world)[1] - D.shard_range(len(origins), r, world)[0] for r in range(world)]
        return D.gather_class_maps(out, counts, dst=0), origins
    return out, origins


def stitch_windows(maps: torch.Tensor, origins: Sequence[Tuple[int, int]], size, fill: int = -1) -> torch.Tensor:
    """Place window class maps back on a (H, W) int8 canvas; pixels no window covers (the remainder strip that the window rule
    drops, e.g. the last 4 px of a 10980 tile) = ``fill``.

    Overlap rule (stride < crop): a pixel takes the prediction of the window whose CENTRE is nearest in the Chebyshev metric
    (predictions are most reliable away from the window border); ties go to the earlier window in row-major order.  The result
    does not depend on the order in which windows are placed."""
    H, W = (size, size) if isinstance(size, int) else size
    crop = maps.shape[-1]
    canvas = torch.full((H, W), fill, dtype=torch.int8, device=maps.device)
    if len(origins) == 0:
        return canvas
    tops = sorted({t for t, _ in origins})
    lefts = sorted({l for _, l in origins})
    grid = len(tops) * len(lefts) == len(origins) and list(origins) == [(t, l) for t in tops for l in lefts]
    step_t = tops[1] - tops[0] if len(tops) > 1 else crop
    step_l = lefts[1] - lefts[0] if len(lefts) > 1 else crop
    regular = all(b - a == crop for a, b in zip(tops, tops[1:])) and all(b - a == crop for a, b in zip(lefts, lefts[1:]))
    if grid and step_t == crop and step_l == crop and regular:
        # non-overlapping regular grid: one strided copy
        ny, nx = len(tops), len(lefts)
        block = maps.view(ny, nx, crop, crop).permute(0, 2, 1, 3).reshape(ny * crop, nx * crop)
        canvas[tops[0] : tops[0] + ny * crop, lefts[0] : lefts[0] + nx * crop] = block
        return canvas
    ax = torch.arange(crop, device=maps.device, dtype=torch.float32) - (crop - 1) / 2.0
    dist = torch.maximum(ax.abs()[:, None], ax.abs()[None, :])  # Chebyshev distance to the window centre (half-integer grid)
    best = torch.full((H, W), float("inf"), dtype=torch.float32, device=maps.device)
    for m, (t, l) in zip(maps, origins):
        reg = best[t : t + crop, l : l + crop]
        take = dist < reg  # strict: ties keep the earlier window
        canvas[t : t + crop, l : l + crop][take] = m[take]
        reg[take] = dist[take]
    return canvas


@torch.no_grad()
def blended_window_inference(tile: torch.Tensor, model, mean: Sequence[float], std: Sequence[float], temporal_size: int = 1,
                             crop_size: int = 224, stride: int = 224, batch_size: int = 64, constant_multiplier: Optional[float] = None,
                             blend: str = "gaussian", sigma_scale: float = 0.125, cover_edges: bool = True,
                             no_data_value: Optional[float] = None, fill: int = -1, probabilities: bool = False, tta: str = "none",
                             uncertainty: bool = False, temperature: float = 1.0) -> Tuple[Optional[torch.Tensor], ...]:
    """tile (T*C, H, W) int16|f32 on the device, any H, W >= crop -> (class map (H, W) int8, probabilities (ncls, H, W) f32 or None)
    on rank 0, (None, None) elsewhere.  A regression head (one output channel) gives (None, the blended value (1, H, W)).

    Windows: the row-major grid of :func:`window_grid` (``cover_edges``: a last row / column of windows at the tile edge).  Every
    window's softmax probabilities are added to the canvas with the weight ``wvec[dy] * wvec[dx]`` (:func:`ops.blend_weights`) and
    divided by the summed weight at the end.  Pixels no window covers, or with any band == ``no_data_value``, get ``fill`` / NaN.
    The canvas is bit-identical for any ``batch_size`` given the same window logits.  Ranks take contiguous blocks of the window
    list (as :func:`sliding_window_inference`) and accumulate only the canvas rows their windows cover; rank 0 adds the bands in
    rank order (:func:`distributed.reduce_row_bands`), which equals the one-rank canvas to fp32 rounding.

    ``tta`` ("none" | "flips" | "d4", :func:`dataloader.d4_codes`): every window is run under K transforms of the square, the logits are
    mapped back and all K enter the canvas with the window's weight.  A forward batch holds whole windows (``max(1, batch_size // K)``
    of them, x K images), so all transforms of a window stay on one rank.  ``uncertainty=True`` returns a third tensor (2, H, W) =
    [normalised entropy, top-two margin] of the blended probabilities on rank 0 (NaN where the class map is ``fill``); a regression
    head has neither and raises ValueError.

    ``temperature`` != 1 multiplies every window's fp32 logits by 1 / temperature in place before they enter the canvas (calibrated
    probabilities, calibration.py); at 1 nothing is multiplied and the canvas keeps its bits.  A blended class map can change with the
    temperature (an average of softmaxes is not monotone in it); a regression head refuses it."""
    codes = d4_codes(tta)
    inv_t = 1.0 / check_temperature(temperature, "temperature")
    net, eng = _engine_of(model)
    net.eval()
    TC, H, W = tile.shape
    ncls = net.cfg.num_classes
    if uncertainty and ncls == 1:
        raise ValueError("uncertainty rasters need class probabilities (a regression head has one output channel)")
    if inv_t != 1.0 and ncls == 1:
        raise ValueError("temperature scaling needs class probabilities (a regression head has one output channel)")
    tops, lefts = window_grid(H, W, crop_size, stride, cover_edges)
    ncol = len(lefts)
    world = D.world_size()
    rank = torch.distributed.get_rank() if world > 1 else 0
    lo, hi = D.shard_range(len(tops) * ncol, rank, world)

    def rows_of(a: int, b: int) -> Tuple[int, int]:  # canvas rows covered by windows [a, b)
        return (tops[a // ncol], tops[(b - 1) // ncol] + crop_size) if b > a else (0, 0)

    if D.dp_active():
        bands = [(y0, y1 - y0) for y0, y1 in (rows_of(*D.shard_range(len(tops) * ncol, r, world)) for r in range(world))]
    else:
        bands = [(0, H)]
    y0, hb = bands[rank]
    dev = tile.device
    canvas = torch.zeros((ncls + 1, hb, W), dtype=torch.float32, device=dev)  # acc (ncls planes) + wsum
    wvec = ops.blend_weights(crop_size, blend, sigma_scale).to(dev)
    tops_d = torch.tensor(tops, dtype=torch.int32).to(dev)
    lefts_d = torch.tensor(lefts, dtype=torch.int32).to(dev)
    mine = origins_tensor([(tops[w // ncol], lefts[w % ncol]) for w in range(lo, hi)], dev)
    n = hi - lo
    C = TC // temporal_size
    K = len(codes)
    per = batch_size if tta == "none" else max(1, batch_size // K)  # windows per forward batch
    nbatch = max(1, -(-n // per))  # balanced batches (sliding_window_inference)
    bs = -(-n // nbatch) if n else 1
    xbuf = torch.empty((max(bs, 1), C, temporal_size, crop_size, crop_size), dtype=torch.float32, device=dev)
    if tta != "none":
        inverse = d4_inverse(codes)
        xk = torch.empty((max(bs, 1) * K, C, temporal_size, crop_size, crop_size), dtype=torch.float32, device=dev)
        back = torch.empty((max(bs, 1) * K, ncls, crop_size, crop_size), dtype=torch.float32, device=dev)
    for i in range(0, n, bs):
        k = min(bs, n - i)
        x, _ = gather_windows(tile, mine[i : i + k], mean, std, temporal_size, crop_size, constant_multiplier, out=xbuf[:k])
        if tta == "none":
            logits = eng.forward(x, training=False, save=False)
            if inv_t != 1.0:
                logits.mul_(inv_t)
            ops.window_blend_accumulate(logits, tops_d, lefts_d, lo + i, wvec, canvas[:ncls], canvas[ncls], H, y0, rows_of(lo + i, lo + i + k))
            continue
        logits = eng.forward(ops.d4_apply(x, codes, True, out=xk[: k * K]), training=False, save=False)
        ops.d4_apply(logits, inverse, False, out=back[: k * K])
        if inv_t != 1.0:
            back[: k * K].mul_(inv_t)
        ops.window_blend_accumulate_tta(back[: k * K].view(k, K, ncls, crop_size, crop_size), tops_d, lefts_d, lo + i, wvec, canvas[:ncls],
                                        canvas[ncls], H, y0, rows_of(lo + i, lo + i + k))
    full = D.reduce_row_bands(canvas, bands, H, dst=0)
    if full is None:
        return (None, None, None) if uncertainty else (None, None)
    out = ops.window_blend_finalize(full[:ncls], full[ncls], tile, no_data_value, fill, probabilities=probabilities)
    if not uncertainty:
        return out
    unc = torch.empty((2, H, W), dtype=torch.float32, device=dev)
    ops.window_blend_uncertainty(full[:ncls], full[ncls], tile, no_data_value, out=unc)
    return out + (unc,)


@torch.no_grad()
def tile_inference(tile_path: str, output_folder: str, model, mean: Sequence[float], std: Sequence[float], temporal_size: int = 1,
                   crop_size: int = 224, stride: int = 224, batch_size: int = 64, constant_multiplier: Optional[float] = None,
                   no_data_value: Optional[float] = -9999, fill: int = -1, device: str = "cuda", blend: str = "nearest",
                   cover_edges: bool = False, sigma_scale: float = 0.125, save_probabilities: bool = False, tta: str = "none",
                   save_uncertainty: bool = False, min_region: int = 0, connectivity: int = 4, sieve_passes: int = 8,
                   save_regions: bool = False, temperature: float = 1.0, zones: Optional[str] = None,
                   zone_id_property: Optional[str] = None, cog: bool = False, cog_blocksize: int = 256, overview_levels="auto",
                   cog_compress: Optional[str] = "deflate", save_polygons: bool = False) -> Optional[str]:
    """GeoTIFF tile -> ``prediction_*.tif`` class map of the same georeferencing: read the (T*C, H, W)
    tile, sliding-window inference over all ranks, stitch, blank NODATA pixels (any band == ``no_data_value``) and uncovered
    border pixels with ``fill``, write on rank 0.  Returns the output path on rank 0, None elsewhere.

    ``blend="nearest"`` (default): square tiles, nearest-centre stitch (:func:`stitch_windows`).  ``blend="mean" | "gaussian"``:
    :func:`blended_window_inference` on any H x W tile, optionally with ``cover_edges``; a regression head writes its blended value
    as float32.  ``save_probabilities`` also writes ``probability_*.tif`` (float32, one band per class, NaN = NODATA); ``tta`` =
    "flips" | "d4" averages every window over its transforms; ``save_uncertainty`` writes ``uncertainty_*.tif`` (float32, band 1 the
    normalised entropy, band 2 the top-two margin of the blended probabilities, NaN = NODATA).

    Products of the finished class map, on either path and on rank 0 (:func:`_write_products`), in map coordinates when the tile is
    georeferenced: ``min_region`` > 0 writes the sieved map as ``prediction_*.tif`` (:func:`postprocess.sieve_class_map` with
    ``connectivity`` and at most ``sieve_passes`` passes); ``save_regions`` writes ``regions_*.csv``, the region table of the written map;
    ``save_polygons`` writes ``polygons_*.geojson``, its regions as polygons with holes (:mod:`instageo_amd.vectorize`); ``zones`` names a
    GeoJSON file of Polygon / MultiPolygon zones in the tile's coordinate system: ``zones_*.csv`` then holds the written map's pixels (and
    map areas) per zone and class (:mod:`instageo_amd.zonal`; rows labelled by the property ``zone_id_property``, else the feature index).
    The probability and uncertainty rasters describe the blend BEFORE the sieve.  With the defaults nothing of this runs.

    ``cog`` writes the class map (after the sieve), ``probability_*.tif`` and ``uncertainty_*.tif`` as Cloud Optimized GeoTIFFs under the
    same names (:mod:`instageo_amd.cog`): tiles of ``cog_blocksize`` (128 | 256 | 512), ``overview_levels`` ("auto" | 0..12) overviews (mode
    with ``fill`` for the class map, NaN-aware mean for the float rasters), ``cog_compress`` "deflate" | "none"; level 0 holds exactly the
    pixels of the strip file.  ``cogstats_*.json`` holds the class histogram of the written map in the reference's form.

    ``temperature`` (blended paths; ``test.temperature`` / ``test.calibration``) calibrates the probabilities that are blended, and
    through them the class map, probability and uncertainty rasters.  The nearest-centre stitch is an argmax of raw logits, which no
    positive temperature changes: it ignores the value."""
    opts = OutputOptions(min_region=min_region, connectivity=connectivity, sieve_passes=sieve_passes, save_regions=save_regions,
                         save_polygons=save_polygons, zones=zones, zone_id_property=zone_id_property, cog=cog, cog_blocksize=cog_blocksize,
                         overview_levels=overview_levels, cog_compress=cog_compress)
    check_temperature(temperature, "temperature")
    opts.check(model)
    if blend not in ("nearest", "mean", "gaussian"):
        raise ValueError(f"blend must be 'nearest', 'mean' or 'gaussian' (got {blend!r})")
    if blend == "nearest" and (cover_edges or save_probabilities):
        raise ValueError("cover_edges and save_probabilities need blend='mean' or 'gaussian' (the nearest-centre stitch has neither)")
    d4_codes(tta)  # an unknown set raises here
    if blend == "nearest" and (tta != "none" or save_uncertainty):
        raise ValueError("tta and save_uncertainty need blend='mean' or 'gaussian' (they work on the probability canvas)")
    arr, profile = tiff.read(tile_path)
    if blend == "nearest" and arr.shape[1] != arr.shape[2]:
        raise ValueError("tile_inference expects a square tile (the window rule of process_test uses one img_size)")
    t = torch.from_numpy(arr if arr.dtype in (np.int16, np.float32) else arr.astype(np.float32)).to(device)
    window = dict(temporal_size=temporal_size, crop_size=crop_size, stride=stride, batch_size=batch_size, constant_multiplier=constant_multiplier)
    if blend == "nearest":
        maps, origins = sliding_window_inference(t, model, mean, std, **window)
        if maps is None:
            return None
        classmap, prob, unc = stitch_windows(maps, origins, tuple(t.shape[1:]), fill), None, None
        if no_data_value is not None:
            classmap[(t == no_data_value).any(0)] = fill
    else:
        res = blended_window_inference(t, model, mean, std, **window, blend=blend, sigma_scale=sigma_scale, cover_edges=cover_edges,
                                       no_data_value=no_data_value, fill=fill, probabilities=save_probabilities, tta=tta,
                                       uncertainty=save_uncertainty, temperature=temperature)
        classmap, prob, unc = (*res, None)[:3]
        if classmap is None and prob is None:
            return None
    # one tail for both paths, on rank 0
    os.makedirs(output_folder, exist_ok=True)
    write = partial(_write_raster, file_name=tile_path, output_folder=output_folder, opts=opts)
    tags = {k: v for k, v in profile["tags"].items() if k != 42113}
    float_prof = dict(profile, count=1, dtype="float32", nodata=None, tags={**tags, 42113: (2, "nan")})
    if classmap is None:  # regression head: the blended value is the prediction
        return write(prob[0], "prediction", "mean", float_prof)
    int_prof = dict(profile, count=1, dtype="int8", nodata=fill, tags=tags)
    ncls = int(getattr(model, "net", model).cfg.num_classes)
    zone_list = zonal.read_zones(zones, zone_id_property) if zones is not None else None
    classmap = _write_products(classmap[None], [(tile_path, int_prof)], output_folder, fill, ncls, opts=opts, zone_list=zone_list)[0]
    out = write(classmap, "prediction", "mode", int_prof, classes=(fill, ncls))
    if prob is not None:
        write(prob, "probability", "mean", dict(float_prof, count=prob.shape[0]))
    if unc is not None:
        write(unc, "uncertainty", "mean", dict(float_prof, count=2))
    return out
