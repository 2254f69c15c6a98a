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
    def __call__(self, images, feature=False):
        """The main head's low-resolution logits; with feature=True `(logits, feature)` of the same run, `feature` is
        the backbone's last tensor, the one FeatureTap takes from the student, as ops.pairwise_kd_loss
        takes it: fp32 [N,C,h,w] from a Seg_Model; from an engine the fp16 [N,h,w,C] view of a contiguous clone of its
        NHWC buffer slice (the pixel pitch may exceed C: the granule's padding is not part of the view)."""
        if not self.is_engine and self.net.training:
            self.net.eval()                 # (a model.train() on an enclosing module must not thaw the BatchNorms)
        # both kinds allocate their result per call (Engine._run, the head's last conv): the caller owns it
        if not feature:
            return self.net.lowres_logits(images)[0]
        if self.is_engine:
            logits, feat, channels = self.net.lowres_logits_and_feature(images)
            return logits, feat[..., :channels]
        got = []
        hook = self.net.backbone.register_forward_hook(lambda mod, args, out: got.append(_last(out)))
        try:
            logits = self.net.lowres_logits(images)[0]
        finally:
            hook.remove()
        return logits, got[0].detach().clone()      # (the caller owns it, as it owns the logits)


def _last(out):
    return out[-1] if isinstance(out, (tuple, list)) else out


class FeatureTap:
    """Takes the student's distilled feature out of a training forward without changing any network's signature: a
    forward hook on `seg_model.backbone` keeps the last tensor the backbone returns - the stage output ASPP / PPM / the
    simple head reads - when grad is enabled and the model is training, and only then.  pop() hands the graph tensor
    out and drops the reference, so that no feature outlives its step."""

    def __init__(self, seg_model):
        if not hasattr(seg_model, "backbone"):
            raise TypeError("FeatureTap: the model has no .backbone")
        self._model, self._kept = seg_model, None
        self._hook = seg_model.backbone.register_forward_hook(self._keep)

    def _keep(self, module, args, out):
        self._kept = _last(out) if (torch.is_grad_enabled() and self._model.training) else None

    def pop(self):
        kept, self._kept = self._kept, None
        return kept

    def remove(self):
        self._hook.remove()
        self._kept = None
