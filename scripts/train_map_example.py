"""MAP training, a KFAC Laplace posterior on the result and its predictive, from files of this repository alone.

    python scripts/train_map_example.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from src.train_map import Adam, cosine_decay_schedule, train_map      # the reference's import path (src/__init__.py)
from lip_amd.kfac import posterior_lla_kfac, predict_lla_kfac
from src.toymodels import SimpleClassifier, create_state

d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "xor.npz"))
x, y = torch.from_numpy(d["x"]), torch.from_numpy(d["y"]).long()
train = [(x[i:i + 128], y[i:i + 128]) for i in range(0, 1024, 128)]
test = [(x[1024:], y[1024:])]
state = create_state(SimpleClassifier(16, 2, 2), seed=0)
state = train_map(state, train, test, model_type="classifier", num_epochs=30, alpha=1e-3,
                  optimizer=Adam(cosine_decay_schedule(1e-2, 30 * len(train), alpha=0.08)), log=print)
posterior = posterior_lla_kfac(state, x[:256], "classifier", alpha=1.0, full_set_size=1024)
mean, var = predict_lla_kfac(state, x[1024:1032], x[:256], "classifier", 1.0, full_set_size=1024, cov="diag")
print("logits", mean[0].tolist(), "variances", var[0].tolist(), "posterior", type(posterior).__name__)
