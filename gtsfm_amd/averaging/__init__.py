"""Averaging stages on the MI355X HIP path."""
