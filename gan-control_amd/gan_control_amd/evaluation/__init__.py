"""What a training run shows for itself: image grids (image_grid.py, generation.py), FID and separability tracking (tracker.py, separability.py)."""
