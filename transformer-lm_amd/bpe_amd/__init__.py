"""bpe_amd -- MI355X-native byte-level BPE, drop-in for gashon/transformer-lm's tokenizer path.

    from bpe_amd import train_bpe, Tokenizer, Vocab

mirror reference models/tokenizer/{train.py, tokenizer.py, vocab.py}.  Compute runs in
libbpe355.so (HIP, gfx950); there is no CPU fallback.
"""
from .train import (train_bpe, train_bpe_bytes, train_bpe_device, last_train_stats,  # noqa: F401
                    set_num_gpus, num_gpus, release_device_memory)
from .counter import WordCounter, train_bpe_files, train_bpe_word_counts  # noqa: F401
from .utf8 import repair_utf8, last_utf8_errors  # noqa: F401
from .vocab import Vocab  # noqa: F401
from .tokenizer import Tokenizer  # noqa: F401


def __getattr__(name):
    # encode_files, id_counts, id_positions live in bpe_amd.encode, which is also run as a script
    # (python -m bpe_amd.encode): imported on first use, not with the package
    if name in ("encode_files", "id_counts", "id_positions"):
        from . import encode
        return getattr(encode, name)
    # the batch loader (bpe_amd.batches) likewise: it needs NumPy, which the tokenizer path does not
    if name in ("load_batch", "TokenStore"):
        from . import batches
        return getattr(batches, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
