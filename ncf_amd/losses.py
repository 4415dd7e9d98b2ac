"""Training objectives next to the reference's ``nn.BCEWithLogitsLoss``
(scripts/train_neumf.py:86), in plain torch: they work on CPU tensors and, through
the module API's autograd (``ncf_amd.ops.ncf_forward``), on the GPU.

The device engine does not call these: ``TrainEngine(loss="bpr")`` forms the same
loss and gradient inside the step kernels (``NCF_DZ_BPR``, include/ncf_hip.h)."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def bpr_loss(pos_logits: torch.Tensor, neg_logits: torch.Tensor) -> torch.Tensor:
    """Bayesian personalised ranking loss of (user, item+, item-) triples:
    mean over triples of -log sigmoid(z+ - z-) = softplus(z- - z+)."""
    if pos_logits.shape != neg_logits.shape:
        raise ValueError("bpr_loss: one negative logit per positive logit")
    return F.softplus(neg_logits - pos_logits).mean()
