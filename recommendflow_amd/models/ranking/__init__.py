"""Ranking models. The trainable rankers over the fused encoder live in their own modules (deepfm, dcn, xdeepfm,
esim_train); TrainableXDeepFM is also exported here, imported on first use so that importing the package stays cheap."""
__all__ = ["TrainableXDeepFM"]


def __getattr__(name):
    if name == "TrainableXDeepFM":
        from .xdeepfm import TrainableXDeepFM

        return TrainableXDeepFM
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
