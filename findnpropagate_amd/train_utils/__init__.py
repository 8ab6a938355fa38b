"""What the reference keeps under tools/train_utils: the optimizer and schedule of its training loop."""
