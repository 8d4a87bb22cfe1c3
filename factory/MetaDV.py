from autoformer_amd.factory.MetaDV import *  # noqa: F401,F403
