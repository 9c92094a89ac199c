"""Generates tests/golden/visualize_golden.npz by RUNNING THE REFERENCE'S OWN CODE: score_to_color_bgr, project_3d_to_2d and
project_all_tracks of visualize.py and normalize_scores of visualizer.py.  Importing either module fails where cv2 is not installed, but
these four functions depend on NumPy only, so the script parses the two files with `ast`, compiles exactly those function definitions and calls
them (as make_sampler_golden.py does).  paint_point_track_with_colors and prepare_video_for_visualization call cv2 and are not run.  No
reference source text is stored: the files are read at generation time only; what is committed are the inputs and the outputs.

Scene: T = 4, N = 24, a 40 x 56 image; per-frame camera matrices (resize 1024 x 1024) and single ones (resize 768 x 1280), with a skew entry;
points behind the camera and points that project far outside the image (clipped).  Colours: -0.3, 0, 0.5, 1, 1.7 and every k / 510, each with
its two fp32 neighbours.  The generator ASSERTS that every projected coordinate is at least 1e-6 away from an integer and from a clip bound, so
that a different double summation order (NumPy's matmul against a left-to-right sum) cannot move a pixel: equality is then required.

    python tests/golden/make_visualize_golden.py <directory of the reference checkout>
"""
import ast
import os
import sys
import warnings

import numpy as np

WANT = {'visualize.py': ('score_to_color_bgr', 'project_3d_to_2d', 'project_all_tracks'), 'visualizer.py': ('normalize_scores',)}
T, N, H, W = 4, 24, 40, 56


def load_reference_functions(ref_dir):
  ns = {'np': np, 'warnings': warnings}
  for fn, names in WANT.items():
    path = os.path.join(ref_dir, fn)
    tree = ast.parse(open(path).read())
    imports = [n for n in tree.body if isinstance(n, ast.ImportFrom) and n.module == 'typing']
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(fns) == len(names), path
    exec(compile(ast.Module(body=imports + fns, type_ignores=[]), path, 'exec'), ns)
  return ns


def unclipped(ref, tracks_tn, K, E, resize):
  """project_all_tracks' steps up to (not including) its clip: [T, N, 2] float64."""
  sx, sy = resize[1] / W, resize[0] / H
  out = np.zeros((T, N, 2))
  for t in range(T):
    k = K[t].copy()
    k[0, 0] *= sx; k[1, 1] *= sy; k[0, 2] *= sx; k[1, 2] *= sy
    c, _ = ref['project_3d_to_2d'](tracks_tn[t], k, E[t])
    out[t, :, 0], out[t, :, 1] = c[:, 0] / sx, c[:, 1] / sy
  return out


def check_margin(u, hi, what):
  inside = (u > 0) & (u < hi)
  d = np.where(inside, np.abs(u - np.rint(u)), np.where(u <= 0, -u, u - hi))
  assert (d >= 1e-6).all(), f'{what}: a coordinate lies within 1e-6 of an integer or of a clip bound: regenerate with another seed'


def main():
  ref = load_reference_functions(sys.argv[1])
  rng = np.random.default_rng(20261018)
  tracks = np.concatenate([rng.uniform(-1.2, 1.2, (N, T, 2)), rng.uniform(1.0, 4.0, (N, T, 1))], -1).astype(np.float32)   # [N, T, 3]
  tracks[3, :, 2] = -2.0          # behind the camera
  tracks[7, 1:3, 2] = -0.7
  tracks[11, :, 0] = 40.0         # far outside: clipped to W - 1
  tracks[12, :, 1] = -35.0        # clipped to 0
  tracks[13, 2] = (-50.0, 60.0, 1.5)
  K1 = np.array([[60.0, 0.3, 28.0], [0.0, 55.0, 20.0], [0.0, 0.0, 1.0]])
  Kt = np.tile(K1[None], (T, 1, 1))
  Kt[:, 0, 0] += np.arange(T) * 1.5
  Kt[:, 1, 2] -= np.arange(T) * 0.75
  Et = np.tile(np.eye(4)[None], (T, 1, 1))
  for t in range(T):
    a = 0.05 * t
    Et[t, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.array([[1, 0, 0], [0, np.cos(0.02), -np.sin(0.02)], [0, np.sin(0.02), np.cos(0.02)]])
    Et[t, :3, 3] = (0.1 * t, -0.05, 0.2)
  E1 = Et[1].copy()
  tn = np.ascontiguousarray(tracks.transpose(1, 0, 2))   # the reference's time-major [T, N, 3]
  out = {'tracks': tracks, 'intrinsics_frames': Kt, 'extrinsics_frames': Et, 'intrinsics_single': K1, 'extrinsics_single': E1, 'hw': np.array([H, W]),
         'resize_frames': np.array([1024, 1024]), 'resize_single': np.array([768, 1280]), 'numpy_version': np.array(np.__version__)}
  for name, K, E, rs in (('frames', Kt, Et, (1024, 1024)), ('single', K1, E1, (768, 1280))):
    got = ref['project_all_tracks'](tn, K.copy(), E.copy(), resize_height=rs[0], resize_width=rs[1], original_height=H, original_width=W)   # [N, T, 2]
    K3, E3 = (K, E) if K.ndim == 3 else (np.tile(K[None], (T, 1, 1)), np.tile(E[None], (T, 1, 1)))
    u = unclipped(ref, tn, K3, E3, rs)
    check_margin(u[..., 0], W - 1, name + ' x')
    check_margin(u[..., 1], H - 1, name + ' y')
    assert np.array_equal(np.clip(u[..., 0], 0, W - 1).T, got[..., 0]) and np.array_equal(np.clip(u[..., 1], 0, H - 1).T, got[..., 1])
    out['tracks_2d_' + name] = got
    # the reference's int() of each coordinate (paint_point_track_with_colors)
    out['pixels_' + name] = np.array([[[int(got[i, t, 0]), int(got[i, t, 1])] for t in range(T)] for i in range(N)], np.int32)
    assert (out['pixels_' + name][..., 0] == W - 1).any() and (out['pixels_' + name][..., 0] == 0).any()
  base = [-0.3, 0.0, 0.5, 1.0, 1.7] + [k / 510 for k in range(511)]
  cs = np.array([v for b in base for v in (np.nextafter(np.float32(b), np.float32(-np.inf)), np.float32(b), np.nextafter(np.float32(b), np.float32(np.inf)))], np.float32)
  out['colour_scores'] = cs
  out['colour_bgr'] = np.array([ref['score_to_color_bgr'](s) for s in cs], np.uint8)
  scores = rng.uniform(-2.0, 5.0, (N, T)).astype(np.float32)
  norm = ref['normalize_scores'](np.ascontiguousarray(scores.T), True)   # the reference's [T, N]
  assert norm.dtype == np.float32
  out['scores'] = scores
  out['scores_norm'] = np.ascontiguousarray(norm.T)
  out['scores_bgr'] = np.array([[ref['score_to_color_bgr'](norm[t, i]) for t in range(T)] for i in range(N)], np.uint8)
  const = np.full((N, T), 0.75, np.float32)
  out['const_norm'] = np.ascontiguousarray(ref['normalize_scores'](np.ascontiguousarray(const.T), True).T)
  out['video'] = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'visualize_golden.npz')
  np.savez_compressed(path, **out)
  print('wrote', path, os.path.getsize(path), 'bytes; numpy', np.__version__)


if __name__ == '__main__':
  main()
