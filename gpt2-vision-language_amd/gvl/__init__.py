"""gvl — MI355X-native hot path of theophile-lt/gpt2-vision-language.

Drop-in module APIs:
    gvl.gpt2       -> source/gpt2/train_gpt2.py model classes (GPT, GPTConfig, Block, ...)
    gvl.caption    -> source/gpt2_linear/model.py and source/gpt2_q_former/model.py
    gvl.cross_att  -> source/gpt2_cross-att/model.py
Runtime:
    gvl.optim (fused AdamW + clip), gvl.dist (bucketed RCCL all-reduce), gvl.train (the
    grad-accumulation DP step), gvl.generate (greedy decode), gvl.decode (KV-cached sampling and
    beam search, speculative decoding; gvl.beam_search and gvl.speculative_generate are
    gvl.decode's), gvl.score (log-probabilities, ranks
    and multiple-choice predictions of given text; gvl.evaluate_hellaswag, gvl.most_likely_row),
    gvl.kernels (C-ABI wrappers), gvl.quant (int8 weight-only decoding: every gvl.decode entry
    point takes weights="int8" or a gvl.quant.quantize_decoder(model) snapshot; the default
    stays bf16).
All compute goes through libgvl.so (include/gvl.h); importing a module that needs it on a
machine without the built library raises at first use, there is no fallback.
"""
import os as _os

__version__ = "0.1.0"
PACKAGE_DIR = _os.path.dirname(_os.path.abspath(__file__))


# KV-cached decoding (gvl.decode), resolved on first use so that `import gvl` stays light.
# (decode.generate is not re-exported: gvl.generate is the full-recompute greedy module.)
_DECODE_NAMES = ("beam_search", "speculative_generate", "KVDecoder", "BeamDecoder",
                 "GraphedGenerate", "GraphedBeamSearch")
# Scoring of given text (gvl.score; gvl.score.score is the function behind the module's name).
_SCORE_NAMES = ("most_likely_row", "evaluate_hellaswag", "Score")


def __getattr__(name):
    if name in _DECODE_NAMES:
        from . import decode
        return getattr(decode, name)
    if name in _SCORE_NAMES:
        from . import score
        return getattr(score, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def library_path():
    from . import _lib
    return _lib.LIB_PATH


def load_library():
    from . import _lib
    return _lib.load()
