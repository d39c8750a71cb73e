"""Config surface of ``run.py`` (reference: ``instageo/model/configs/*.yaml`` + Hydra ``key=value`` overrides).

Hydra/OmegaConf are not available offline, so the same keys are provided as plain dictionaries: ``DEFAULTS``
carries every key of the reference's ``config.yaml``; ``PRESETS[name]`` holds the values in which
``--config-name name`` differs.  Values are the reference's published recipe constants (data, not code).
"""
from __future__ import annotations

import copy
from typing import Any, Dict, List

DEFAULTS: Dict[str, Any] = {'root_dir': None,
 'valid_filepath': None,
 'train_filepath': None,
 'test_filepath': None,
 'checkpoint_path': None,
 'mode': 'train',
 'is_reg_task': False,
 'train': {'learning_rate': 0.0001,
           'num_epochs': 10,
           'batch_size': 8,
           'class_weights': [1, 1],
           'ignore_index': -100,
           'weight_decay': 0.01,
           'scheduler': False,
           'distillation': False,
           'teacher_ckpt_path': None,
           # segmentation objective (not in the reference): ce | focal | dice | ce_dice | focal_dice (segmentation.loss_spec)
           'loss': 'ce',
           'focal_gamma': 2.0,
           'region_weight': 1.0,
           'region_smooth': 1.0,
           'tversky': [0.5, 0.5]},
 'model': {'model_name': 'prithvi_eo_tiny',
           'freeze_backbone': False,
           'load_pretrained_weights': True,
           'num_classes': 2,
           'use_log_scale': False,
           'plot_reg_results': False,
           'include_ee_metric': False,
           'weight_clip_range': None,
           'depth': -1},
 'dataloader': {'bands': [1, 2, 3, 8, 11, 12],
                'mean': [0.14245495, 0.13921481, 0.12434631, 0.31420089, 0.20743526, 0.12046503],
                'std': [0.04036231, 0.04186983, 0.05267646, 0.0822221, 0.06834774, 0.05294205],
                'img_size': 224,
                'temporal_dim': 1,
                'replace_label': [-1, 2],
                'reduce_to_zero': False,
                'no_data_value': -9999,
                'constant_multiplier': 1.0,
                'max_pixel_value': 10000,
                'num_workers': 1,
                'augmentations': {'hflip': {'use': True, 'p': 0.5},
                                  'vflip': {'use': True, 'p': 0.5},
                                  'rotate': {'use': True, 'p': 0.5, 'degrees': 10},
                                  'brightness': {'use': True,
                                                 'p': 0.5,
                                                 'brightness_range': [0.8, 1.2],
                                                 'contrast_range': [0.8, 1.2]},
                                  'blur': {'use': True, 'p': 0.5, 'kernel_size': 3, 'sigma_range': [0.1, 2.0]},
                                  'noise': {'use': True, 'p': 0.5, 'noise_std': 0.05}}},
 'test': {'img_size': 224, 'crop_size': 224, 'stride': 224, 'mask_cloud': False,
          # mode=tile_inference (not in the reference): window blending of the tile path; the defaults are the nearest-centre stitch
          'blend': 'nearest', 'cover_edges': False, 'sigma_scale': 0.125, 'save_probabilities': False,
          # blended modes only: test-time augmentation over the flips ('flips') or all of D4 ('d4'), entropy / margin raster
          'tta': 'none', 'save_uncertainty': False,
          # chip / tile inference (not in the reference): sieve of regions below min_region pixels (0 = off) under 4- or 8-connectivity
          # with at most sieve_passes passes, and the region table regions_*.csv (postprocess.py)
          'min_region': 0, 'connectivity': 4, 'sieve_passes': 8, 'save_regions': False,
          # the regions of the written class map as polygons_*.geojson, traced on the device under `connectivity` (vectorize.py)
          'save_polygons': False,
          # zonal statistics (not in the reference): a GeoJSON FeatureCollection of Polygon / MultiPolygon zones in the raster's coordinate
          # system (None = off); zones_*.csv then counts the pixels of every class of the written class map inside every zone, rasterised
          # and tallied on the device (zonal.py).  zone_id_property: the feature property to label the rows with (None = the feature index)
          'zones': None, 'zone_id_property': None,
          # Cloud Optimized GeoTIFF output of mode=tile_inference (cog.py): the class map, probability and uncertainty rasters become tiled
          # GeoTIFFs with overviews built on the device (same file names; level 0 holds the same pixels) and cogstats_*.json holds the class
          # histogram.  cog_blocksize: 128 | 256 | 512 (the reference's BLOCKSIZE=chip_size); overview_levels: 'auto' (until both sides
          # fit a block) or 0..12 (the reference asks for 6); cog_compress: 'deflate' | 'none'
          'cog': False, 'cog_blocksize': 256, 'overview_levels': 'auto', 'cog_compress': 'deflate',
          # mosaic of mode=chip_inference (not in the reference's run.py; its serving layer runs gdal_merge): after the chips are written,
          # rank 0 pastes the prediction_*.tif files on their common grid on the device and writes predictions_merged.tif with the region /
          # polygon / zone products of the whole map (mosaic.py).  mosaic_rule: where chips overlap, 'last' | 'first' file in name order,
          # 'mode' (class maps) or 'mean' (regression); mosaic_cog: a COG with cogstats_merged.json under the cog_blocksize /
          # overview_levels / cog_compress keys, else a strip file; mosaic_cover: also cover_merged.tif, the chips that cover each pixel
          'mosaic': False, 'mosaic_rule': 'last', 'mosaic_cog': True, 'mosaic_cover': False,
          # one mosaic across coordinate systems (warp.py): mosaic_crs None = one mosaic per coordinate system, 'first' = the first
          # chip's, or 'EPSG:n' (UTM zones, 3857, 4326); mosaic_resolution: the target pixel size, None = the first chip's;
          # mosaic_resampling: None = nearest for class maps and bilinear for regression, or 'nearest' | 'bilinear'
          'mosaic_crs': None, 'mosaic_resolution': None, 'mosaic_resampling': None,
          # calibrated probabilities (not in the reference): logits / temperature in front of every softmax consumer (predict_step, the
          # blended tile canvas, the test epoch's ROC-AUC).  temperature: a float > 0, None = 1.0 (nothing is scaled); calibration: the
          # calibration.json of mode=calibrate to take it from (one of the two).  calibration_metrics: mode=eval also logs test_nll /
          # test_ece / test_mce at the temperature in force
          'temperature': None, 'calibration': None, 'calibration_metrics': False,
          # boundary quality (not in the reference): mode=eval also logs test_bIoU_d<d> (Boundary IoU, with _<class>), test_trimap_Acc_d<d>
          # and test_trimap_IoU_d<d> over the pixels within d pixels of a class boundary, for each of up to 8 ascending distances in
          # [1, 32] (boundary.py)
          'boundary_metrics': False, 'boundary_distances': [1, 2, 4],
          # object level (not in the reference): mode=eval also logs test_obj_F1_t<t> / test_obj_P_t<t> / test_obj_R_t<t> (detection of the
          # connected regions at IoU > t; F1 with _<class>) and test_PQ_t<t> (with _<class>) / test_SQ_t<t> / test_RQ_t<t> (panoptic
          # quality) for each of up to 10 ascending thresholds in [0.5, 0.999] of at most three decimals.  object_connectivity: 4 | 8;
          # object_min_area: regions below it in pixels are neither objects nor matches; object_classes: the classes the means run over
          # (None = all) (objects.py)
          'object_metrics': False, 'object_iou_thresholds': [0.5], 'object_connectivity': 4, 'object_min_area': 1, 'object_classes': None,
          # Web Mercator map tiles (not in the reference's run.py; its backend serves them through TiTiler; maptiles.py): map_tiles writes
          # tiles_<name>/{z}/{x}/{y}.png + tilejson.json of the class map / prediction raster of mode=tile_inference, and tiles_merged/ of
          # the mosaic of mode=chip_inference (test.mosaic=true), rendered on the device.  map_tiles_minzoom / map_tiles_maxzoom: 'auto' or
          # 0..24; map_tiles_size: the tile side, a multiple of 64 in 64..1024; map_tiles_palette: a JSON file of [r, g, b(, a)] entries
          # (the class colours, or the 256 entries of the regression ramp); map_tiles_rescale: [lo, hi] of the ramp, None = the finite
          # minimum and maximum; map_tiles_imagery: also tiles_chips/ (+ chips_merged.tif) from the input chips; map_tiles_png_level: 0..9.
          # mode=map_tiles renders the existing GeoTIFF test.input into <its folder>/tiles_<name>/
          'map_tiles': False, 'map_tiles_minzoom': 'auto', 'map_tiles_maxzoom': 'auto', 'map_tiles_size': 256, 'map_tiles_palette': None,
          'map_tiles_rescale': None, 'map_tiles_imagery': False, 'map_tiles_png_level': 6, 'input': None},
 # mode=calibrate (not in the reference): temperature fit on valid_filepath -- grid points per pass, passes, the first grid's range,
 # bins of the reliability histograms (calibration.py)
 'calibrate': {'points': 32, 'passes': 2, 't_min': 0.125, 't_max': 8.0, 'nbins': 15},
 # mode=create_chips (the reference's instageo/data chip creator under its flag names; chips.py): tiles = the HLS band files ordered per
 # date and band (B02_0, B03_0, ...), fmasks = one Fmask file per date (None: no masking), records_file = the CSV of x, y, label, date
 # (None: every complete chip of the grid, for inference), output_directory = where chips/, seg_maps/ and the dataset CSV go
 'chips': {'chip_size': 256, 'mask_types': [], 'masking_strategy': 'each', 'window_size': 0, 'task_type': 'seg', 'src_crs': 4326,
           'tiles': None, 'fmasks': None, 'records_file': None, 'output_directory': None},
 # mode=create_s2_chips (the reference's S2PointsPipeline of instageo/data/s2_utils.py; s2_chips.py): tiles = the Sentinel-2 L2A band files
 # (GeoTIFF / COG) ordered per date and band, each on its own grid (10 m, 20 m, 60 m) with one shared top-left corner; scl = one scene
 # classification file per date (None: no masking); mask_types = names of SCL classes (cloud, water, cloud_shadow, cirrus, snow),
 # mask_classes = further class numbers 0..31; spatial_resolution = the chips' pixel size in metres (None: that of the first band file);
 # boa_offset = subtracted from every non-zero value (1000 for processing baseline >= 04.00; 0: the reference); valid_range = [lo, hi]
 # outside which a value becomes 0 (None: no check); granule_id = the product name the tile id is taken from (None: from the first file
 # name); records_file = the CSV of x, y, label, date (None: every complete chip of the grid, for inference)
 's2_chips': {'chip_size': 256, 'mask_types': [], 'mask_classes': [], 'masking_strategy': 'each', 'window_size': 0, 'task_type': 'seg',
              'src_crs': 4326, 'spatial_resolution': None, 'boa_offset': 0, 'valid_range': None, 'tiles': None, 'scl': None,
              'granule_id': None, 'records_file': None, 'output_directory': None},
 # mode=create_raster_chips (the reference's instageo/data/raster_chip_creator.py under its flag names; raster_chips.py): every label is a
 # raster of chip_size x chip_size pixels in EPSG:src_crs at spatial_resolution, listed in records_file (a CSV of label_filename, date
 # [, mgrs_tile_id]) and found under raster_path; the stack of tiles / fmasks is resampled onto each label's grid.  is_bbox_feature: no
 # labels, chips over the boxes of the JSON list bbox_feature_path, named by date.  Not in the reference: snap (true: the lattice of
 # multiples of spatial_resolution, as stackstac resamples; false: the label raster's own grid)
 'raster_chips': {'tiles': None, 'fmasks': None, 'records_file': None, 'raster_path': None, 'output_directory': None, 'chip_size': 256,
                  'mask_types': [], 'masking_strategy': 'each', 'src_crs': 4326, 'spatial_resolution': 0.0002694945852358564,
                  'qa_check': True, 'task_type': 'seg', 'is_bbox_feature': False, 'bbox_feature_path': None, 'date': None, 'snap': True},
 # mode=create_s2_raster_chips (the reference's S2RasterPipeline of instageo/data/s2_utils.py, the default source of raster_chip_creator.py;
 # s2_raster_chips.py): tiles / scl / mask_types / mask_classes / boa_offset / granule_id as in s2_chips (the band files may lie on grids of
 # any corner), records_file / raster_path / chip_size / src_crs / spatial_resolution / snap / qa_check as in raster_chips.  valid_range =
 # [lo, hi] outside which a value becomes 0 ([0, 10000]: the reference always applies it here; None: no check).  is_bbox_feature: no labels,
 # records_file is then the JSON list of boxes and the chips are named by the granule's date
 's2_raster_chips': {'tiles': None, 'scl': None, 'records_file': None, 'raster_path': None, 'output_directory': None, 'chip_size': 256,
                     'mask_types': [], 'mask_classes': [], 'masking_strategy': 'each', 'src_crs': 4326,
                     'spatial_resolution': 0.0002694945852358564, 'snap': True, 'qa_check': True, 'is_bbox_feature': False, 'boa_offset': 0,
                     'valid_range': [0, 10000], 'granule_id': None},
 # mode=create_s1_chips (the reference's S1PointsPipeline of instageo/data/s1_utils.py; s1_chips.py): scenes = the Sentinel-1 RTC band files
 # (float32 GeoTIFF / COG) as a list of dates, each a list of scenes (the slices of the orbit, tried in order), each a list of one file per
 # band ([[[a_vv.tif, a_vh.tif]], [[b1_vv.tif, b1_vh.tif], [b2_vv.tif, b2_vh.tif]]]; a date written as one flat list is one scene);
 # epsg = the coordinate system of the stack (None: the first scene's), spatial_resolution = its pixel size; no_data_value = the fill and
 # the no-data value of the chips (-1: NO_DATA_VALUES.S1), src_nodata = the files' own no-data value (None: only NaN), clip = [lo, hi] for
 # present values (None: the reference, which does not clip); records_file = the CSV of x, y, label, date (None: every complete chip)
 's1_chips': {'scenes': None, 'records_file': None, 'output_directory': None, 'chip_size': 256, 'bands': ['vv', 'vh'],
              'masking_strategy': 'each', 'window_size': 0, 'task_type': 'seg', 'src_crs': 4326, 'epsg': None, 'spatial_resolution': 10,
              'no_data_value': -1, 'src_nodata': None, 'clip': None},
 # mode=create_s1_raster_chips (not in the reference, which has no label-raster pipeline for Sentinel-1; s1_raster_chips.py): scenes / bands /
 # no_data_value / src_nodata / clip as in s1_chips (cut dB scenes with no_data_value=-9999: -1.0 is a valid dB value), records_file /
 # raster_path / chip_size / src_crs / spatial_resolution / snap / qa_check / task_type / is_bbox_feature / bbox_feature_path / date as in
 # raster_chips; tile_id = the id of the names and of the records this run takes (None: from the first file's name)
 's1_raster_chips': {'scenes': None, 'records_file': None, 'raster_path': None, 'output_directory': None, 'chip_size': 256,
                     'bands': ['vv', 'vh'], 'masking_strategy': 'each', 'src_crs': 4326, 'spatial_resolution': 0.0002694945852358564,
                     'qa_check': True, 'task_type': 'seg', 'is_bbox_feature': False, 'bbox_feature_path': None, 'date': None, 'snap': True,
                     'no_data_value': -1, 'src_nodata': None, 'clip': None, 'tile_id': None},
 # mode=create_composite (not in the reference, which takes one scene per temporal step; composite.py): scenes = the HLS band files of one
 # MGRS tile as a list of steps, each a list of scenes, each a list of one file per band ([[[a_B02.tif, a_B03.tif], [b_B02.tif, b_B03.tif]]]);
 # fmasks = the same nesting without the band level, one Fmask file per scene (None: only no_data decides what is clear); dates = one target
 # date per step, the candidates are tried by distance from it (None: the date of the step's first scene, list order kept); method = nearest
 # (the nearest clear date), median (per band the lower median of the clear values) or medoid (the clear scene closest to the median
 # spectrum); mask_types = the Fmask types that make an observation not clear; a pixel with fewer than min_clear clear observations gets
 # no_data; device: None = the device when there is one, host, cuda
 'composite': {'scenes': None, 'fmasks': None, 'dates': None, 'method': 'medoid',
               'mask_types': ['cloud', 'near_cloud_or_shadow', 'cloud_shadow'], 'min_clear': 1, 'no_data': -9999, 'output_directory': None,
               'device': None},
 # mode=filter_s1 (not in the reference, which neither filters speckle nor converts to dB; s1_filter.py): scenes = Sentinel-1 RTC band
 # files (float32) in the nesting of s1_chips.scenes, or one flat list; each is written under the same base name into output_directory,
 # ready to be named in s1_chips.scenes.  method = boxcar, lee or gamma_map over a window x window neighbourhood (odd, 3..15), or refined_lee
 # (edge-aligned half windows; window must be 7), looks = the
 # equivalent number of looks (4.4: IW GRD), scale = linear or db (cut dB chips with s1_chips.no_data_value=-9999: -1.0 is a valid dB
 # value), src_nodata = the files' own no-data value (None: each file's no-data tag)
 's1_filter': {'scenes': None, 'output_directory': None, 'method': 'lee', 'window': 7, 'looks': 4.4, 'scale': 'linear', 'src_nodata': None},
 # mode=filter_s1_temporal (not in the reference; s1_temporal.py): scenes = the Sentinel-1 RTC band files (float32) of a stack in the nesting
 # of s1_chips.scenes, dates of scenes of one file per band; every date is filtered by borrowing the other dates at the same pixel (Quegan
 # and Yu's multi-temporal filter on a window x window local mean, odd, 3..15) and written under the same base name into output_directory,
 # ready to be named in s1_chips.scenes or s1_filter.scenes.  Files are grouped per band by coordinate system and pixel lattice; a file
 # alone on its lattice comes back unfiltered.  scale = linear or db, src_nodata = the files' own no-data value (None: each file's tag)
 's1_temporal': {'scenes': None, 'output_directory': None, 'bands': ['vv', 'vh'], 'window': 7, 'scale': 'linear', 'src_nodata': None},
 # mode=clean_chips (the reference's instageo/data/data_cleaner.py under its flag names; clean.py): drop the chips of chips_dataset_csv
 # whose share of no-data pixels is above the threshold, buffer the observation pixels of the label maps by window_size (or limit the maps
 # to the pixels of observation_points_csv), write output_chips_dataset_csv and clean_stats.json.  Not in the reference: num_classes
 # (cells of the class histogram; None: the largest label + 1) and root_dir (where relative paths of the CSV start; None: the CSV's folder)
 'clean': {'chips_dataset_csv': None, 'output_chips_dataset_csv': None, 'drop_chips': False, 'drop_chips_strategy': 'any',
           'no_data_threshold': 0.5, 'no_data_value': -9999, 'clean_seg_maps': False, 'cleaning_method': 'buffer',
           'observation_points_csv': None, 'seg_map_output_dir': None, 'ignore_index': -1, 'window_size': 1, 'num_classes': None,
           'root_dir': None},
 # mode=create_polygon_labels (not in the reference, which expects label rasters made with GDAL; polygon_labels.py): the polygons of the
 # GeoJSON `features` (EPSG:src_crs) are burned into labels/label_x{x}_y{y}_{date}.tif of chip_size x chip_size pixels + records.csv, the
 # input of mode=create_raster_chips.  The grid is that of the raster `like` (an HLS tile: the labels sit on its pixels), else EPSG:crs
 # (None: the UTM zone of the features) at spatial_resolution.  The value of a feature: its value_property (an integer, or a name looked
 # up in class_map) or the constant burn_value; later features win; background: what no feature covers (None: 0 for seg, NaN for reg);
 # labelled_area: a GeoJSON outside which pixels get the ignore value; date or date_property name the rasters; a cell with fewer than
 # min_foreground labelled pixels is dropped; device: None = the device when there is one, host, cuda
 'polygon_labels': {'features': None, 'output_directory': None, 'like': None, 'crs': None, 'src_crs': 4326, 'spatial_resolution': 30.0,
                    'chip_size': 256, 'task_type': 'seg', 'value_property': None, 'burn_value': None, 'class_map': None, 'background': None,
                    'labelled_area': None, 'date': None, 'date_property': None, 'mgrs_tile_id': None, 'min_foreground': 1, 'device': None},
 # mode=zonal_stats (not in the reference; zonal.py): per zone and band the count, mean, std, min, max and sum of the GeoTIFF `raster`
 # (any sample type, float32 on the device: a prediction, probability or uncertainty raster, a Sentinel-1 dB scene, a composite) over the
 # Polygon / MultiPolygon features of the GeoJSON `zones`, written as the CSV `output` (None: zonevalues_<raster base name>.csv next to
 # the raster).  zone_id_property: the property that names a zone (None: its index); bands: a list of band indices (None: all); nodata:
 # the value that marks missing samples (None: the file's own no-data tag; NaN and Inf are always missing); zones_crs: the EPSG code of
 # the zones' coordinates (None: those of the raster)
 'zonal_stats': {'raster': None, 'zones': None, 'zone_id_property': None, 'output': None, 'bands': None, 'nodata': None,
                 'zones_crs': None},
 # mode=split_dataset (the step of the reference's instageo/data/data_splitter.py under its flag names where they exist, on a rule of this
 # project's own; split.py): the rows of the dataset CSV input_file go to output_dir/splits/train.csv, val.csv and test.csv by whole
 # spatial clusters (strategy kmeans: n_clusters, max_iter), whole years (year) or at random (random), seeded by random_state;
 # include_val / include_test = false skip a set.  Not in the reference: buffer_km (the guard band: train rows nearer than that to a val
 # or test row, then val rows nearer than that to a test row, are left out; 0 removes nothing), max_iter, root_dir (where relative paths
 # of the CSV start; None: the CSV's folder), save_geojson (splits.geojson, one Point per row) and device: None = the device when there
 # is one, host, cuda
 'split': {'input_file': None, 'output_dir': None, 'test_ratio': 0.2, 'val_ratio': 0.2, 'include_val': True, 'include_test': True,
           'random_state': 42, 'n_clusters': 20, 'strategy': 'kmeans', 'buffer_km': 0.0, 'max_iter': 100, 'root_dir': None,
           'save_geojson': True, 'device': None}}

PRESETS: Dict[str, Dict[str, Any]] = {'sen1floods11': {'train': {'batch_size': 16, 'class_weights': [1, 3], 'ignore_index': -1},
                  'model': {'model_name': 'prithvi_eo_v1_100'},
                  'dataloader': {'replace_label': None,
                                 'augmentations': {'rotate': {'use': False},
                                                   'brightness': {'use': False},
                                                   'blur': {'use': False},
                                                   'noise': {'use': False}}},
                  'test': {'img_size': 512}},
 'multitemporal_crop_classification': {'train': {'class_weights': [0.386375,
                                                                   0.661126,
                                                                   0.548184,
                                                                   0.640482,
                                                                   0.876862,
                                                                   0.925186,
                                                                   3.249462,
                                                                   1.542289,
                                                                   2.175141,
                                                                   2.272419,
                                                                   3.062762,
                                                                   3.626097,
                                                                   1.198702],
                                                 'ignore_index': -1},
                                       'model': {'model_name': 'prithvi_eo_v1_100', 'num_classes': 13},
                                       'dataloader': {'bands': [0,
                                                                1,
                                                                2,
                                                                3,
                                                                4,
                                                                5,
                                                                6,
                                                                7,
                                                                8,
                                                                9,
                                                                10,
                                                                11,
                                                                12,
                                                                13,
                                                                14,
                                                                15,
                                                                16,
                                                                17],
                                                      'mean': [494.905781,
                                                               815.239594,
                                                               924.335066,
                                                               2968.881459,
                                                               2634.621962,
                                                               1739.579917],
                                                      'std': [284.925432,
                                                              357.84876,
                                                              575.566823,
                                                              896.601013,
                                                              951.900334,
                                                              921.407808],
                                                      'temporal_dim': 3,
                                                      'replace_label': None,
                                                      'reduce_to_zero': True,
                                                      'no_data_value': None}},
 'locust': {'train': {'num_epochs': 20, 'ignore_index': -1, 'weight_decay': 0.1},
            'model': {'model_name': 'prithvi_eo_v1_100'},
            'dataloader': {'bands': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17],
                           'mean': [623.2724609375,
                                    1247.657958984375,
                                    1772.24169921875,
                                    2371.256103515625,
                                    2862.867431640625,
                                    2357.759765625],
                           'std': [2182.050048828125,
                                   2248.420654296875,
                                   2302.53515625,
                                   2372.204345703125,
                                   2398.52685546875,
                                   2292.96435546875],
                           'temporal_dim': 3,
                           'replace_label': [-9999, -1],
                           'augmentations': {'rotate': {'use': False},
                                             'brightness': {'use': False},
                                             'blur': {'use': False},
                                             'noise': {'use': False}}}}}
PRESETS["config"] = {}


def _merge(dst: Dict[str, Any], src: Dict[str, Any]) -> Dict[str, Any]:
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = v
    return dst


def _parse_value(text: str) -> Any:
    import yaml

    try:
        return yaml.safe_load(text)
    except Exception:
        return text


def load_config(config_name: str = "config", overrides: List[str] = (), config_path: str = None) -> Dict[str, Any]:
    """``--config-name`` preset (or a YAML file under ``--config-path``) + ``a.b.c=value`` / ``+key=value`` overrides."""
    cfg = copy.deepcopy(DEFAULTS)
    if config_path:
        import os

        import yaml

        path = os.path.join(config_path, config_name if config_name.endswith((".yaml", ".yml")) else config_name + ".yaml")
        _merge(cfg, yaml.safe_load(open(path)) or {})
    elif config_name not in PRESETS:
        raise KeyError(f"unknown config {config_name!r}; available: {sorted(PRESETS)}")
    else:
        _merge(cfg, copy.deepcopy(PRESETS[config_name]))
    for ov in overrides:
        if "=" not in ov:
            raise ValueError(f"override {ov!r} is not key=value")
        key, val = ov.split("=", 1)
        add = key.startswith("+")
        key = key.lstrip("+")
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            if p not in node:
                if not add:
                    raise KeyError(f"unknown config key {key!r} (use +{key}=... to add)")
                node[p] = {}
            node = node[p]
        if parts[-1] not in node and not add:
            raise KeyError(f"unknown config key {key!r} (use +{key}=... to add)")
        node[parts[-1]] = _parse_value(val)
    return cfg


def check_required_flags(required: List[str], cfg: Dict[str, Any]) -> None:
    """pipeline_utils.py:44-55: a flag counts as missing when it is None or the *string* "None"."""
    for flag in required:
        if cfg.get(flag) is None or cfg.get(flag) == "None":
            raise RuntimeError(f"Flag --{flag} is required.")
