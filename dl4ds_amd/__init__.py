"""dl4ds_amd -- MI355X-native drop-in for the conv-SR train-step path of carlos-gg/dl4ds.

Mirrors the reference's public names for that path (dl4ds/__init__.py:7-45): the constants below are
reproduced verbatim; ``models``, ``training``, ``inference``, ``losses`` and ``utils`` expose the same
builder / trainer signatures.  All arithmetic runs in libdl4ds_hip.so (hand-written gfx950 kernels);
there is no CPU fallback.
"""
__version__ = '0.1.0'

BACKBONE_BLOCKS = [
    'convnet',          # plain convolutional block w/o skip connections
    'resnet',           # residual convolutional blocks
    'densenet',         # dense convolutional blocks
    'convnext',         # convnext style residual blocks
    'unet']             # unet (encoder-decoder) backbone

UPSAMPLING_METHODS = [
    'spc',              # pixel shuffle or subpixel convolution in post-upscaling
    'rc',               # resize convolution in post-upscaling
    'dc',               # deconvolution or transposed convolution in post-upscaling
    'pin']              # pre-upsampling via (bicubic) interpolation
POSTUPSAMPLING_METHODS = ['spc', 'rc', 'dc']

INTERPOLATION_METHODS = ['inter_area', 'nearest', 'bicubic', 'bilinear', 'lanczos']

LOSS_FUNCTIONS = ['mae', 'mse', 'dssim', 'dssim_mae', 'dssim_mse', 'dssim_mae_mse',
                  'msdssim', 'msdssim_mae', 'msdssim_mae_mse']

DROPOUT_VARIANTS = ['vanilla', 'gaussian', 'spatial', 'mcdrop', 'mcgaussiandrop', 'mcspatialdrop']


def __getattr__(name):
    # lazy: importing the package must not need the GPU library (tests/test_abi.py runs on CPU)
    import importlib
    lazy = {'SupervisedTrainer': '.training', 'CGANTrainer': '.training', 'Predictor': '.inference', 'compute_metrics': '.metrics',
            'compute_rmse': '.metrics', 'compute_correlation': '.metrics',
            'StandardScaler': '.preprocessing', 'MinMaxScaler': '.preprocessing',
            'predict': '.inference', 'predict_ensemble': '.inference', 'EnsemblePredictor': '.inference',
            'verify_ensemble': '.inference', 'EnsembleVerifier': '.inference', 'ensemble_scores': '.metrics',
            'exceedance_scores': '.metrics', 'verify_exceedance': '.inference', 'ExceedanceVerifier': '.inference',
            'multivariate_scores': '.metrics', 'verify_multivariate': '.inference', 'MultivariateVerifier': '.inference',
            'neighbourhood_scores': '.metrics', 'fss': '.metrics',
            'neighbourhood_ensemble_scores': '.metrics', 'verify_neighbourhood': '.inference',
            'NeighbourhoodVerifier': '.inference',
            'sal_from_objects': '.objects', 'check_object_args': '.objects',
            'label_objects': '.objects', 'sal_scores': '.objects', 'object_scores': '.objects',
            'distance_transform': '.distance', 'distance_scores': '.distance', 'distance_from_sums': '.distance',
            'check_distance_args': '.distance',
            'Regridder': '.regrid', 'regrid': '.regrid', 'axis_table': '.regrid', 'check_regrid_args': '.regrid',
            'consistency_scores': '.regrid', 'consistency_from_sums': '.regrid',
            'distribution_scores': '.metrics', 'quantile_maps': '.metrics',
            'spectral_scores': '.metrics', 'power_spectrum': '.metrics',
            'QuantileMapper': '.postprocessing', 'quantile_map': '.postprocessing', 'check_qmap_args': '.postprocessing',
            'predict_tiled': '.inference', 'TiledPredictor': '.inference', 'plan_tiles': '.tiling',
            'climate_indices': '.indices', 'precipitation_indices': '.indices', 'temperature_indices': '.indices',
            'percentile_threshold': '.indices', 'index_scores': '.indices', 'check_index_args': '.indices',
            'temporal_statistics': '.temporal', 'temporal_scores': '.temporal', 'temporal_from_sums': '.temporal',
            'mann_kendall': '.temporal', 'trend_scores': '.temporal', 'check_temporal_args': '.temporal',
            'l_moments': '.extremes', 'block_maxima': '.extremes', 'peaks_over_threshold': '.extremes',
            'lmoments_from_pwm': '.extremes', 'gev_from_lmoments': '.extremes', 'gumbel_from_lmoments': '.extremes',
            'gpd_from_lmoments': '.extremes', 'return_levels': '.extremes', 'fit_gev': '.extremes', 'fit_gumbel': '.extremes',
            'fit_gpd': '.extremes', 'extreme_scores': '.extremes', 'check_extreme_args': '.extremes',
            'net_postupsampling': '.models', 'net_pin': '.models', 'unet_pin': '.models',
            'recnet_postupsampling': '.models', 'recnet_pin': '.models', 'residual_discriminator': '.models',
            'DataGenerator': '.dataloader', 'create_batch_hr_lr': '.dataloader', 'create_pair_hr_lr': '.dataloader',
            'crop_array': '.dataloader', 'resize_array': '.dataloader', 'checkarray_ndim': '.dataloader',
            'spatial_to_spatiotemporal_samples': '.utils', 'spatiotemporal_to_spatial_samples': '.utils',
            'checkarg_backbone': '.utils', 'checkarg_upsampling': '.utils', 'checkarg_loss': '.utils',
            'checkarg_dropout_variant': '.utils', 'check_compatibility_upsbackb': '.utils'}
    if name in lazy:
        return getattr(importlib.import_module(lazy[name], __name__), name)
    raise AttributeError(name)
