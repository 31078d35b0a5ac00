"""Which ATen ops of a whole-model training step have no deterministic form: one step (320x240,
B = 2, float32 and bf16 autocast) under torch.use_deterministic_algorithms(True, warn_only=True),
with rgbd_amd.determinism's switch on and off, printing the distinct warnings."""
import sys
import warnings
from pathlib import Path
R = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(R), str(R / "tests"), str(R / "tests" / "golden")]
import torch
import _rgbd_import  # noqa: F401
import golden_inputs as gi
from rgbd_amd import determinism, init as winit
from rgbd_amd.config import standard_config
from rgbd_amd.custom_model import CustomMask2FormerForUniversalSegmentation
DEV = torch.device("cuda", 0)
torch.manual_seed(0)
m = CustomMask2FormerForUniversalSegmentation(standard_config(48), version="0.4.0")
winit.init_deterministic(m)
m = m.to(DEV).train()
H, W, B = 240, 320, 2
pv = torch.from_numpy(gi.pixel_values(6, B, H, W)).to(DEV)
masks, classes = gi.labels(6, B, H, W)
ml = [torch.from_numpy(x).to(DEV) for x in masks]
cl = [torch.from_numpy(c).to(DEV) for c in classes]
for switch in (True, False):
    for amp in (False, True):
        m.set_compute_dtype(torch.bfloat16 if amp else torch.float32)
        m.zero_grad(set_to_none=True)
        torch.use_deterministic_algorithms(True, warn_only=True)
        determinism.set_deterministic(switch)
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter("always")
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                out = m(pixel_values=pv, mask_labels=ml, class_labels=cl)
            out.loss.backward()
            torch.cuda.synchronize()
        torch.use_deterministic_algorithms(False)
        msgs = sorted({str(w.message).split(". You can")[0][:200] for w in ws if "deterministic" in str(w.message)})
        print(f"switch={switch} amp={amp} loss={float(out.loss.detach())!r}: {len(msgs)} nondeterministic-op warnings")
        for s in msgs:
            print("   ", s)
