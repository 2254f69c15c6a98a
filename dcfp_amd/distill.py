"""The frozen teacher of the distillation fine-tune.

The fine-tune stage trains the slim model that tools/prune.py cut out of the dense checkpoint.  `Teacher` holds that
dense model, frozen, next to the student and hands its main-head low-resolution logits to loss.CriterionKD as
labels['teacher']:

    teacher = Teacher.from_checkpoint(dense_model, "dense.pth").to(device)
    labels = {"ori": labels, "teacher": teacher(images)}
    loss = student(images, labels)            # criterion 'ce,kd' / 'gsrl,kd'

Why the engine is the default.  A Seg_Model teacher runs the training code's fp32 inference convs, and each of those
registers a permuted copy of its weight tensor with ops (ops._wp_buffer).  ops.refresh_wp(), which every optimizer
step runs, rebuilds ALL registered copies in its one launch - the frozen teacher's too, on every step, although its
weights never change.  deploy.build_engine packs the teacher's weights once into an fp16 engine that is outside that
registry, owns no nn.Parameter (nothing an optimizer or a parameter arena could pick up) and runs the forward about
four times faster than the fp32 path.  Its logits carry fp16 rounding; a teacher is a soft target, not a reference.
`engine=False` keeps the fp32 model for comparisons."""
import torch

from . import deploy
from .utils.pyt_utils import load_model


class Teacher:
    """A frozen network that maps images to the fp32 low-resolution logits of its main head.

    net: an eval-mode Seg_Model (its parameters are detached from autograd here: requires_grad False, so that no
    optimizer built over `requires_grad` parameters and no parameter arena adopts them) or a deploy.Engine."""

    def __init__(self, net):
        self.is_engine = isinstance(net, deploy.Engine)
        if not self.is_engine:
            if not isinstance(net, torch.nn.Module) or not hasattr(net, "lowres_logits"):
                raise TypeError("Teacher: net must be a Seg_Model or a deploy.Engine")
            net.eval()
            for p in net.parameters():
                p.requires_grad_(False)
        self.net = net

    @classmethod
    def from_checkpoint(cls, model, path, engine=True):
        """Load the weights at `path` (a state_dict file or the dict itself) into `model` (on the CPU, built like the
        checkpoint's network) and wrap it: frozen into an fp16 engine (the default, see the module docstring) or as the
        fp32 model itself."""
        load_model(model, path)
        model.eval()
        return cls(deploy.build_engine(model) if engine else model)

    def to(self, device):
        self.net = self.net.to(device)
        return self

    def parameters(self):
        """The nn.Parameters behind the teacher (none for an engine): what must never reach an optimizer."""
        return [] if self.is_engine else list(self.net.parameters())

    @torch.no_grad()
    def __call__(self, images):
        if not self.is_engine and self.net.training:
            self.net.eval()                 # (a model.train() on an enclosing module must not thaw the BatchNorms)
        # both kinds allocate their result per call (Engine._run, the head's last conv): the caller owns it
        return self.net.lowres_logits(images)[0]
