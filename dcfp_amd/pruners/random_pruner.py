"""Random channel pruning - the baseline criterion of the reference's `pruners` package, on the static ChannelPruner.

Every prunable conv draws one uniform number per output channel and keeps the channels whose number exceeds
`global_percent`, so a share of about `global_percent` goes, with no regard to the weights.  It exists to be compared
against: DCFP-pruned + fine-tune against random-pruned + fine-tune at the same FLOPs (tools/prune.py --prune-type
random)."""
import torch

from .channel_pruner import ChannelPruner


def random_out_masks(norm_conv_links, except_layers, channels, global_percent, layer_keep, generator=None):
    """{conv name: float mask [C]} for the convs of `norm_conv_links` (BN name -> conv name) outside `except_layers`:
    mask = rand(C) > global_percent; a layer left with fewer than max(1, int(C * layer_keep)) channels keeps its first
    that many as well.  Layers are visited in the order of `norm_conv_links`, each drawing C numbers from `generator`."""
    masks = {}
    for bn, conv in norm_conv_links.items():
        if conv in except_layers:
            continue
        n = channels[bn]
        min_keep = max(1, int(n * layer_keep))
        mask = (torch.rand(n, generator=generator) > global_percent).float()
        if int(mask.sum()) < min_keep:
            mask[:min_keep] = 1.0
        masks[conv] = mask
    return masks


class RandomChannelPruner(ChannelPruner):
    def __init__(self, global_percent=0.8, layer_keep=0.01, except_start_keys=("head.fc",), seed=None, **kwards):
        super().__init__(except_start_keys=list(except_start_keys))
        self.layer_keep = layer_keep
        self.global_percent = global_percent
        # seed None: torch's global generator, as the reference draws; an int makes the cut repeatable
        self.generator = None if seed is None else torch.Generator().manual_seed(int(seed))

    def gen_channel_mask(self):
        channels = {bn: self.name2module[bn].weight.data.shape[0] for bn in self.norm_conv_links}
        masks = random_out_masks(self.norm_conv_links, self.except_layers, channels, self.global_percent,
                                 self.layer_keep, self.generator)
        for conv, mask in masks.items():
            m = self.name2module[conv]
            m.out_mask = mask.reshape(m.out_mask.shape)
