"""Head widths at the boundary (no compute, no GPU): the last block of the readout stack runs the single-query attention kernels (csrc/model.hip block_fwd_last ->
csrc/attn_q1.hip) in every precision, for both model kinds and whatever attn_impl says, and those exist for qkv_size / num_heads in {8, 16, 32, 64, 96, 128} only.
Any other width is refused where the model is created -- SPA3D_ERR_ARG from spa3d_create, ValueError from the Python model -- instead of a HIP-class error at the
first forward of a handle that was created successfully."""
import ctypes as C

import pytest

from util import MINI, O, product_model

SUPPORTED = (8, 16, 32, 64, 96, 128)
ERR_ARG = 1


@pytest.fixture(scope='module')
def spa3d():
  import spa3d as s
  return s


def _create(spa3d, heads, qkv, precision, kind):
  L = spa3d._lib
  cfg = L.Config(MINI['num_output_frames'], MINI['num_latent_tokens'], MINI['latent_token_dim'], MINI['num_frequencies'], 1.0, 1.0, MINI['track_token_dim'],
                 MINI['encoder_latent_dim'], MINI['decoder_num_channels'], 0, 0, heads, qkv, MINI['enc_mlp'], MINI['enc_layers'], MINI['t2l_mlp'],
                 MINI['t2l_layers'], MINI['dec_mlp'], MINI['dec_layers'], MINI['ro_mlp'], MINI['ro_layers'], precision, kind)
  h = C.c_void_p()
  rc = L.load().spa3d_create(C.byref(cfg), C.byref(h))
  if rc == 0:
    L.load().spa3d_destroy(h)
  return rc


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('precision', [0, 1, 2])
def test_create_accepts_the_six_head_widths_and_refuses_the_others(spa3d, precision, kind):
  for Dh in range(1, 129):
    for heads in (1, 2):
      rc = _create(spa3d, heads, heads * Dh, precision, kind)
      assert rc == (0 if Dh in SUPPORTED else ERR_ARG), (Dh, heads, rc)
  assert _create(spa3d, 2, 2 * 132, precision, kind) == ERR_ARG and _create(spa3d, 1, 256, precision, kind) == ERR_ARG


@pytest.mark.parametrize('heads,qkv', [(2, 48), (1, 40), (4, 192), (3, 12), (1, 4)])
def test_python_model_raises_value_error_before_create(spa3d, heads, qkv):
  cfg = O.Config(**{**MINI, 'num_heads': heads, 'qkv_size': qkv}, use_dino=False, use_depth=False)
  for precision in ('fp32', 'bf16', 'fp16'):
    m = product_model(spa3d, cfg, precision)
    with pytest.raises(ValueError, match='head width'):
      m._handle(0, 0)


def test_python_model_accepts_the_six_head_widths(spa3d):
  for Dh in SUPPORTED:
    cfg = O.Config(**{**MINI, 'num_heads': 2, 'qkv_size': 2 * Dh}, use_dino=False, use_depth=False)
    h, leaves, n = product_model(spa3d, cfg, 'bf16')._handle(0, 0)
    assert h and n > 0
