"""Developer benchmark of BASELINE configs[4]: one DINOv2 student/teacher iteration (ssl.SSLTrainer) of the hybrid octic
ViT-H/16 on 2 x 224^2 + 8 x 96^2 crops per image, bf16 autocast, synthetic crops resident in HBM.
usage: bench_ssl.py [images_per_gpu=32] [steps=5] [centering=centering|sinkhorn_knopp] [fused_sinkhorn=1|0] [head_hip=1|0]
                    [dino_head_hip=1|0]
(fused_sinkhorn=0: the Sinkhorn-Knopp targets as the eager composition, every other row kernel of the losses unchanged;
head_hip=0: ssl.HEAD_HIP off - the input rows of the DINO / iBOT head calls as new_zeros + index_select + copy_ + cat;
dino_head_hip=0: ssl.DINO_HEAD_HIP off - the heads themselves as the stock torch composition on the BLAS library)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from octic_vits_amd import ssl as S
from octic_vits_amd.dinov2_models import hybrid_dinov2_vit_huge_patch16

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
centering = sys.argv[3] if len(sys.argv) > 3 else "centering"
fused_sinkhorn = bool(int(sys.argv[4])) if len(sys.argv) > 4 else True
S.HEAD_HIP = bool(int(sys.argv[5])) if len(sys.argv) > 5 else True
S.DINO_HEAD_HIP = bool(int(sys.argv[6])) if len(sys.argv) > 6 else True
if not fused_sinkhorn:
    S.sinkhorn_fused_ok = lambda teacher_output, n_iterations: False
torch.manual_seed(0)
arch = S.SSLMetaArch(lambda: hybrid_dinov2_vit_huge_patch16(img_size=224, drop_path_rate=0.4), 1280, centering=centering).cuda()
tr = S.SSLTrainer(arch, lr=1e-4)
images = S.synthetic_multicrop_batch(batch, "cuda", seed=5)
for _ in range(2):
    out = tr.step(images, teacher_temp=0.04, momentum=0.992)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    out = tr.step(images, teacher_temp=0.04, momentum=0.992)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
print(f"ssl step ({centering}{'' if fused_sinkhorn else ', Sinkhorn-Knopp as the eager composition'}{'' if S.HEAD_HIP else ', HEAD_HIP off'}{'' if S.DINO_HEAD_HIP else ', DINO_HEAD_HIP off'}): {batch} images/GPU ({2 * batch} global + {8 * batch} local crops): "
      f"{dt * 1e3:.1f} ms/step, {batch / dt:.1f} images/s, "
      f"peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB, losses " + ", ".join(f"{k}={float(v):.3f}" for k, v in out.items()))
