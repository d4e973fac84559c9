"""Drop-in for the reference's `mhb_coAtt` module (train_models.py:9)."""
from _pkg import pkg as _p


class MHBCoAtt(_p.MHBCoAtt):
    """The package's MHBCoAtt behind exactly the reference's forward signature (mhb_coAtt.py:61); the shared-image call form
    (`img_index`) lives on the package class, `vqa_amd.MHBCoAtt`."""

    def forward(self, img_features, questions, glove_matrix=None, is_training=True):
        return super().forward(img_features, questions, glove_matrix, is_training)


MHB = _p.MHB
