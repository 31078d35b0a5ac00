"""The Hugging Face ``Trainer`` (the reference's training loop, finetuning.py:98) with its
gradient clip on the HIP kernels: ``Trainer._clip_grad_norm`` — accelerate's clip_grad_norm_, i.e.
torch.nn.utils.clip_grad_norm_ over ``model.parameters()`` with ``args.max_grad_norm`` (1.0 unless
set) — becomes ``rgbd_amd.optim.clip_grad_norm_``: norm, finalise and in-place scale, three kinds
of launch instead of torch's foreach norm / stack / norm / multiply over every tensor.  Nothing
else of the Trainer changes; ``HipClipTrainer(..., args=TrainingArguments(max_grad_norm=1.0))``
trains as ``Trainer`` does.  float32 gradients on one GPU per process (the reference's DDP set-up)."""
from transformers import Trainer

from .optim import clip_grad_norm_


class HipClipTrainer(Trainer):
    def _clip_grad_norm(self, model):
        """Clip gradients to max_grad_norm; returns the pre-clip norm (a 0-d device tensor)."""
        self.accelerator.unscale_gradients()  # as accelerate's clip_grad_norm_ does (no-op without a GradScaler)
        return clip_grad_norm_(model.parameters(), self.args.max_grad_norm)
