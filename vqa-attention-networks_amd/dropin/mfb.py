"""Drop-in for the reference's `mfb` module: `mfb.MFB(cfg)` on the MI355X HIP path."""
from _pkg import pkg as _p


class MFB(_p.MFB):
    """The package's MFB behind exactly the reference's forward signature (mfb.py:61); the shared-image call form
    (`img_index`) lives on the package class, `vqa_amd.MFB`."""

    def forward(self, img_features, questions, is_training=True):
        return super().forward(img_features, questions, is_training)
