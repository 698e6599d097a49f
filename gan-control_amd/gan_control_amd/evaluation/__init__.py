"""What a training run shows for itself: image grids (image_grid.py, generation.py) and FID tracking (tracker.py)."""
