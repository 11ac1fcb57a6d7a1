"""The DPT depth head on a GPU machine: it has no GPU path (octic_vits_amd/depth.py, NOTES 'DPT depth head'), so what is checked
here is that nothing of it is launched on the device - a head moved to the GPU or a GPU tensor is refused by DPTHead.forward,
DPTHead.forward_tokens and, before the backbone runs, by DepthEncoderDecoder - while the linear head beside it still takes GPU
tensors and the DPT head still answers on the CPU of the same machine."""
import os
from functools import partial

import numpy as np
import pytest
import torch

import cases
import dpt_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    from octic_vits_amd import depth, dinov2_vit
    m = dinov2_vit.DinoVisionTransformer(block_fn=partial(dinov2_vit.Block, attn_class=dinov2_vit.MemEffAttention), block_chunks=0,
                                         **PC.SPEC)
    cases.fill_parameters(m, salt=PC.SALT)
    model = depth.dpt_depther(m, out_index=PC.OUT_INDEX, min_depth=PC.MIN_DEPTH, max_depth=PC.MAX_DEPTH).eval()
    PC.fill_head(model.decode_head)
    return model


def test_gpu_tensors_and_a_head_on_the_gpu_are_refused_and_the_cpu_still_answers():
    model = _model()
    head = model.decode_head
    g = torch.Generator().manual_seed(0)
    pairs = [(torch.randn(2, 12, 64, generator=g), torch.randn(2, 64, generator=g)) for _ in range(4)]
    gpu_pairs = [(p.to(DEV), c.to(DEV)) for p, c in pairs]
    with torch.no_grad():
        want = head.forward_tokens(pairs, (3, 4))
        for call in (lambda: head.forward_tokens(gpu_pairs, (3, 4)),                      # GPU tokens, head on the CPU
                     lambda: head.forward([(p.reshape(2, 3, 4, 64).permute(0, 3, 1, 2), c) for p, c in gpu_pairs])):
            with pytest.raises(RuntimeError, match="no GPU path"):
                call()
        head.to(DEV)
        try:
            with pytest.raises(RuntimeError, match="no GPU path"):                        # CPU tokens, head on the GPU
                head.forward_tokens(pairs, (3, 4))
        finally:
            head.cpu()
        assert torch.equal(head.forward_tokens(pairs, (3, 4)), want)


def test_the_encoder_decoder_refuses_before_its_backbone_runs_and_the_golden_holds_on_this_machines_cpu():
    model = _model()
    ran = []
    real = model.backbone.get_intermediate_layers
    model.backbone.get_intermediate_layers = lambda *a, **k: (ran.append(1), real(*a, **k))[1]
    x = PC.image()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no GPU path"):
            model.whole_inference(x.to(DEV), None, True)
        assert not ran
        got = model.whole_inference(x, None, False).numpy()
    assert ran
    want = np.load(os.path.join(ROOT, "tests", "golden", "dpt_head.npz"))["whole_raw"]
    assert float(np.abs(got.astype(np.float64) - want).max()) <= 9 * 256 * 2.0 ** -24 * float(np.abs(want).max())
