"""MXDESK_VP8_TOKENS (EncoderConfig.vp8_tokens): who boolean-codes the VP8 token partitions."""
import pytest

from mxdesk.utils import config as C


@pytest.mark.parametrize("value", ["host", "gpu"])
def test_vp8_tokens_env_accepted(value):
    assert C.load(env={"MXDESK_VP8_TOKENS": value}, argv=[]).vp8_tokens == value


def test_vp8_tokens_default_is_host():
    assert C.load(env={}, argv=[]).vp8_tokens == "host"


@pytest.mark.parametrize("value", ["cpu", "1", ""])
def test_vp8_tokens_env_rejected(value):
    with pytest.raises(ValueError, match="MXDESK_VP8_TOKENS"):
        C.load(env={"MXDESK_VP8_TOKENS": value}, argv=[])


def test_vp8_tokens_encoder_config_defaults(native):
    cfg = native.EncoderConfig()
    assert cfg.vp8_tokens == -1 and cfg.vp8_tokens_cap == 1024
