"""Shim package: ``realesrgan.archs`` (upstream's network definitions) for the drop-in import lines."""
