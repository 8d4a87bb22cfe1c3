from autoformer_amd.melgan import Audio2Mel, Generator, ResnetBlock, WNConv1d, WNConvTranspose1d  # noqa: F401
