"""Re-export of physicsinformeddiffusionmodels_amd.mechanics_data_generation next to the reference's module paths (the reference
has no generator for its mechanics data); `python -m src.mechanics_data_generation` runs its main()."""
from physicsinformeddiffusionmodels_amd.mechanics_data_generation import *  # noqa: F401,F403
from physicsinformeddiffusionmodels_amd import mechanics_data_generation as _m

globals().update({k: v for k, v in vars(_m).items() if not k.startswith('__')})

if __name__ == "__main__":
    _m.main()
