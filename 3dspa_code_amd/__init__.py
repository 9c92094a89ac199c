"""3dspa_code_amd -- MI355X-native (gfx950) 3DSPA TrackAutoEncoder3D train-step hot path.

The directory name is not a Python identifier; import it as `import spa3d` (repo-root shim) or
`importlib.import_module('3dspa_code_amd')`."""
from . import _lib
from .model import (LossConfig, POS_L1, POS_HUBER, ParamTree, TrackAutoEncoder, TrackAutoEncoder3D, compute_loss_2d, TrackAutoEncoderDecoderContext, TrackAutoEncoderResults, compute_loss_3d,
                    profile_summary, sinusoidal_embedding, SampleScores, TrackScores, VideoScores, score_predictions, TapVid3DScores, TapVid3DSampleScores,
                    tapvid3d_predictions, evaluate_tapvid3d, aggregate_tapvid3d, render_tracks, render_heatmap, project_tracks, visualize_npz)
from .data import build_batch, build_windows, stitch_windows, window_starts, collate_ragged, draw_split, fold_offsets, convert_predictions_to_tapvid3d_format, load_checkpoint, split_ragged, load_train_state, prepare_3d_batch, save_checkpoint, save_scores_npz
from .motion import KernelDistance, ManifoldMetrics, MotionStats, frechet_distance, kernel_distance, limbs_to_ints, manifold_metrics, motion_kernel_sums, motion_ball_hits, motion_codes, motion_knn, motion_pdist, precision_recall
from .features import lift_2d_to_3d, sample_depth_features_for_tracks, sample_dino_features_for_tracks
from .train import ParamGroups, TrainState, allreduce_flat_, create_learning_rate_schedule, global_visible_count, param_groups

__all__ = ['LossConfig', 'POS_L1', 'POS_HUBER', 'TrackAutoEncoder3D', 'TrackAutoEncoder', 'compute_loss_2d', 'TrackAutoEncoderResults', 'TrackAutoEncoderDecoderContext', 'ParamTree', 'compute_loss_3d',
           'sinusoidal_embedding', 'profile_summary', 'lift_2d_to_3d', 'sample_dino_features_for_tracks',
           'sample_depth_features_for_tracks', 'prepare_3d_batch', 'convert_predictions_to_tapvid3d_format', 'load_checkpoint',
           'save_checkpoint', 'load_train_state', 'TrainState', 'param_groups', 'ParamGroups','create_learning_rate_schedule', 'global_visible_count', 'allreduce_flat_', 'collate_ragged', 'split_ragged', 'build_batch', 'build_windows', 'stitch_windows', 'window_starts', 'draw_split', 'fold_offsets', 'TrackScores', 'VideoScores', 'SampleScores', 'score_predictions', 'save_scores_npz', 'TapVid3DScores', 'TapVid3DSampleScores', 'tapvid3d_predictions',
           'MotionStats', 'frechet_distance', 'motion_codes', 'motion_pdist', 'precision_recall', 'motion_knn', 'motion_ball_hits', 'manifold_metrics', 'ManifoldMetrics', 'motion_kernel_sums', 'limbs_to_ints', 'kernel_distance', 'KernelDistance', 'evaluate_tapvid3d', 'aggregate_tapvid3d', 'render_tracks', 'render_heatmap', 'project_tracks', 'visualize_npz', '_lib']
