"""The numpy restatement of the denoising filter (tests/denoise_reference.py) checked against what the filter must do by construction.
No GPU: the device is compared with the restatement in tests/test_denoise_gpu.py."""
from denoise_reference import (test_a_constant_image_comes_back_unchanged,  # noqa: F401
                               test_nothing_crosses_an_instance_boundary,
                               test_with_all_stops_open_an_iteration_is_the_plain_b3_convolution)
