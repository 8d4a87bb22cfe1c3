from autoformer_amd.factory.LstmDV import *  # noqa: F401,F403
