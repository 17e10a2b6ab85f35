"""Re-export of physicsinformeddiffusionmodels_amd.darcy_data_generation under the reference's module path
(src/darcy_data_generation.py); `python -m src.darcy_data_generation` runs its main()."""
from physicsinformeddiffusionmodels_amd.darcy_data_generation import *  # noqa: F401,F403
from physicsinformeddiffusionmodels_amd import darcy_data_generation as _m

globals().update({k: v for k, v in vars(_m).items() if not k.startswith('__')})

if __name__ == "__main__":
    _m.main()
