"""Ranking models. The trainable rankers over the fused encoder live in their own modules (deepfm, dcn, xdeepfm,
tabtransformer, esim_train); TrainableXDeepFM and TrainableTabTransformer are also exported here, imported on first use so
that importing the package stays cheap."""
__all__ = ["TrainableXDeepFM", "TrainableTabTransformer"]


def __getattr__(name):
    if name == "TrainableXDeepFM":
        from .xdeepfm import TrainableXDeepFM

        return TrainableXDeepFM
    if name == "TrainableTabTransformer":
        from .tabtransformer import TrainableTabTransformer

        return TrainableTabTransformer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
