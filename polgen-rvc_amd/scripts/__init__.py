"""Mirrors of the reference's ``rvc/scripts`` modules that run on the GPU."""
